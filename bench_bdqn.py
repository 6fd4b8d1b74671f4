"""Branching DQN at the examples/box2d/bipedal_bdq.py shape (record, not a gate): obs 24, common [512, 256], value [128], action
[128], D = 4 branches of A = 25 actions, B = 512, Adam, target network, double Q-learning -- the engine beside the same update in
eager PyTorch on the same GPU, in one process.

    python bench_bdqn.py [--steps K] [--warmup W] [--out profiles/bdqn_bench.json]

One "update" = `target_q` on the next observations (online and lagged network, per-branch argmax, the mean over the branches)
and the update proper (forward, loss, reverse pass, one Adam step); the lagged network is synchronised every
TARGET_UPDATE_FREQ-th update on both sides.  The eager baseline is the reference's target and update (bdqn.py:155-224) written
out below on the stand-in BranchingNet of tests/standin_bdqn.py moved to the device, with torch.optim.Adam.  Both are timed in
alternation, each call on its own with a device synchronisation, after a clock warm-up; the figure is the median of the timed
calls.  No ratio is fixed in advance.  `launches_per_update` counts the launches the engine's route issues from its own code
(the GEMM layer may add helper launches of its own inside a call).  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

OBS, COMMON, VALUE_H, ACTION_H, D, A, BATCH = 24, (512, 256), 128, 128, 4, 25, 512
GAMMA, LR, TARGET_UPDATE_FREQ = 0.99, 1e-4, 1000                          # bipedal_bdq.py's defaults


def _stats(times: list[float]) -> dict:
    med = statistics.median(times)
    q = statistics.quantiles(times, n=4)
    return {"updates_per_s_median": 1.0 / med, "updates_per_s_min": 1.0 / max(times), "updates_per_s_max": 1.0 / min(times),
            "ms_per_update_median": med * 1e3, "ms_per_update_q1": q[0] * 1e3, "ms_per_update_q3": q[2] * 1e3}


def _eager(params: dict):
    """The reference's target and update restated on the stand-in modules -> a callable."""
    import copy

    from tests import standin_bdqn as SM

    net = SM.BranchingNet(state_shape=OBS, num_branches=D, action_per_branch=A, common_hidden_sizes=list(COMMON),
                          value_hidden_sizes=[VALUE_H], action_hidden_sizes=[ACTION_H])
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.copy_(params[k])
    net = net.cuda()
    old = copy.deepcopy(net)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    it = [0]

    def one(obs, act, obs_next, rew, end):
        with torch.no_grad():                                               # bdqn.py:155-195
            a_star = net(obs_next)[0].argmax(-1, keepdim=True)
            boot = old(obs_next)[0].gather(-1, a_star).squeeze(-1).mean(-1)
            ret = rew + GAMMA * boot * (1.0 - end)
        if it[0] % TARGET_UPDATE_FREQ == 0:                                 # dqn.py:277-285
            old.load_state_dict(net.state_dict())
        it[0] += 1
        q = net(obs)[0]                                                     # bdqn.py:211-222
        mask = torch.zeros_like(q).scatter_(-1, act.unsqueeze(-1), 1)
        td = ret.view(-1, 1, 1) * mask - q * mask
        loss = td.pow(2).sum(-1).mean(-1).mean()
        prio = td.sum(-1).sum(-1)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item(), prio

    return one


def launches_per_update(n_common: int, relu: bool = True) -> dict:
    """What ts_bdqn_target_q (double, lagged network) and ts_bdqn_update enqueue from their own code, ReLU fused into the GEMMs."""
    act = 0 if relu else 1
    fwd = n_common * (1 + act) + (1 + act) + 1                              # common layers, the fan, the head kernel
    target = 1 + 2 * fwd + 1                                                # pad, two passes, the target kernel
    per = 3 + act                                                           # wgrad, slab sum, dgrad (ReLU mask inside; tanh: + one launch)
    bwd = 4 + per + (n_common - 1) * per + 2                                # head bwd / finish / head wgrad / slab sum; fan; layers; layer 1
    update = 1 + fwd + bwd + 1                                              # pad, forward, reverse, Adam (no clip)
    return {"target_q": target, "update": update, "total": target + update}


def run(steps: int, warmup: int) -> dict:
    import bench_init as BI
    from tests import oracle_bdqn as OB
    from tianshou_amd import bdqn as BD

    dims = BD.make_dims(OBS, COMMON, VALUE_H, ACTION_H, D, A, "relu")
    params = OB.random_params(dims, 0)
    cfg = BD.BDQNConfig(gamma=GAMMA, target_update_freq=TARGET_UPDATE_FREQ, is_double=True, lr=LR)
    eng = BD.BDQNEngine(*dims, BD.flat_from_torch([params[k] for k in BD.state_keys(dims)], *dims, "cuda"), cfg)
    eager = _eager(params)
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randn(BATCH, OBS, generator=g, device="cuda")
    obs_next = torch.randn(BATCH, OBS, generator=g, device="cuda")
    act = torch.randint(0, A, (BATCH, D), generator=g, device="cuda")
    rew = torch.randn(BATCH, generator=g, device="cuda")
    end = (torch.rand(BATCH, generator=g, device="cuda") < 0.05).float()

    def engine_update():
        loss, prio = eng.update(obs, act, eng.target_q(obs_next, rew, end))
        return loss.item()

    def eager_update():
        return eager(obs, act, obs_next, rew, end)[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    first = (timed(engine_update)[1], timed(eager_update)[1])                # the same parameters and batch: the same loss
    BI.warm_clocks()
    n, warm = max(steps, 20), max(warmup, 3)
    order = [(engine_update, []), (eager_update, [])]
    for i in range(warm + n):
        k = i % len(order)
        for fn, sink in order[k:] + order[:k]:                              # rotate who goes first
            dt, _ = timed(fn)
            if i >= warm:
                sink.append(dt)
    se, sg = (_stats(t) for _, t in order)
    return {
        "metric": "BDQN engine-level updates/sec (bipedal_bdq.py shape, B=512)",
        "value": se["updates_per_s_median"], "unit": "updates/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic", "higher_is_better": True,
        "config": {"workload": f"obs {OBS}, common {list(COMMON)}, value [{VALUE_H}], action [{ACTION_H}], D={D}, A={A}, B={BATCH}, Adam lr {LR}, "
                               f"target network (freq {TARGET_UPDATE_FREQ}), double; one update = target_q on obs_next + update",
                   "eager": "the same target and update on tests/standin_bdqn.py modules on the same GPU, torch.optim.Adam, fp32"},
        "engine_target_q_plus_update": se, "eager_same_gpu": sg, "timed_updates": n, "warmup": warm,
        "engine_ms": se["ms_per_update_median"], "eager_ms": sg["ms_per_update_median"],
        "engine_vs_eager": se["updates_per_s_median"] / sg["updates_per_s_median"],
        "engine_not_slower_than_eager": se["ms_per_update_median"] <= sg["ms_per_update_median"],
        "launches_per_update": launches_per_update(len(COMMON)), "first_loss_engine_eager": list(first), "parameters": eng.count,
    }


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bdqn_bench.json"))
    a = ap.parse_args()
    res = run(a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
