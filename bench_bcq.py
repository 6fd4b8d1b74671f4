"""DiscreteBCQ on the C3 shape (record, not a gate): 84x84x4 uint8 observations, 6 actions, 1-step returns, lagged net, at
B = 512 and at B = 32 (the batch size of examples/offline/atari_bcq.py) -- beside the DQN engine on the same inputs and the
same update in eager PyTorch on the same GPU, all three in one process.

    python bench_bcq.py [--steps K] [--warmup W] [--out profiles/bcq_bench.json]

One "update" = the target pass on s' (live trunk + both live heads, lagged trunk + Q head, masked argmax), the 1-step return,
and the update on s (forward, three-term loss, backward through both heads into the shared trunk, Adam).  The DQN engine runs
its own target pass (two trunks, two heads) and its own update on the same tensors: BCQ has one more 512-wide head in each
direction of the update and one more in the target pass.  The eager baseline is the same BCQ update on the stand-in modules of
tests/standin_bcq.py moved to the device, with torch.optim.Adam.  The three are timed in alternation, each update on its own
with a device synchronisation, after a clock warm-up; the figure is the median of the timed updates.  Two conditions are
checked and reported: BCQ must not be slower than the eager update, and the ratio to DQN is recorded (DESIGN.md explains it
from the launch list).  Prints one JSON line and writes it to --out.
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

C, H, W, N_ACT = 4, 84, 84, 6
GAMMA, LR, FREQ, TAU, THETA = 0.99, 6.25e-5, 8000, 0.3, 1e-2


def _stats(times: list[float]) -> dict:
    med = statistics.median(times)
    q = statistics.quantiles(times, n=4)
    return {"updates_per_s_median": 1.0 / med, "updates_per_s_min": 1.0 / max(times), "updates_per_s_max": 1.0 / min(times),
            "ms_per_update_median": med * 1e3, "ms_per_update_q1": q[0] * 1e3, "ms_per_update_q3": q[2] * 1e3}


def _eager(batch: int):
    """The reference's update restated on the stand-in modules (discrete_bcq.py:104-127, 228-261) -> a callable."""
    import copy

    import torch.nn.functional as F

    from tests import standin_bcq as SB

    torch.manual_seed(0)
    trunk = SB.DQNetFeaturesOnly(C, H, W)
    model, imitator = (SB.DiscreteActor(preprocess_net=trunk, action_shape=N_ACT, hidden_sizes=[512], softmax_output=False)
                       for _ in range(2))
    policy = SB.DiscreteBCQPolicy(model=model, imitator=imitator, unlikely_action_threshold=TAU).cuda()
    old = copy.deepcopy(policy.model)
    opt = torch.optim.Adam(policy.parameters(), lr=LR)
    inf = torch.finfo(torch.float32).max
    rows = torch.arange(batch, device="cuda")

    def forward(obs):
        q, _ = policy.model(obs)
        lg, _ = policy.imitator(obs)
        ratio = lg - lg.max(dim=-1, keepdim=True).values
        return q, lg, (q - inf * (ratio < policy._log_tau).float()).argmax(dim=-1)

    def one(obs, obs_next, act, rew, mask):
        with torch.no_grad():
            _, _, a = forward(obs_next)
            tq = old(obs_next)[0][rows, a]
            ret = rew + GAMMA * mask * tq
        q, lg, _ = forward(obs)
        q_loss = F.smooth_l1_loss(q[rows, act], ret)
        i_loss = F.nll_loss(F.log_softmax(lg, dim=-1), act)
        reg_loss = lg.pow(2).mean()
        loss = q_loss + i_loss + THETA * reg_loss
        opt.zero_grad()
        loss.backward()
        opt.step()
        return torch.stack([loss.detach(), q_loss.detach(), i_loss.detach(), reg_loss.detach()]).tolist()      # as the four .item() calls

    return one


def run_batch(batch: int, steps: int, warmup: int) -> dict:
    import bench_init as BI
    from oracle import oracle_dqn as OD
    from tests import oracle_bcq as OB
    from tianshou_amd import bcq as BQ
    from tianshou_amd import dqn as D

    p = OB.init_params(C, H, W, N_ACT, 0)
    bcq = BQ.BCQEngine(C, H, W, N_ACT, BQ.flat_from_torch([p[k] for k in OB.PARAM_ORDER], C, H, W, N_ACT),
                       BQ.BCQConfig(gamma=GAMMA, n_step=1, target_update_freq=FREQ, unlikely_action_threshold=TAU,
                                    imitation_logits_penalty=THETA, lr=LR))
    pd = OD.init_params(C, H, W, N_ACT, 0)
    dqn = D.DQNEngine(C, H, W, N_ACT, D.flat_from_torch([pd[k] for k in OD.PARAM_ORDER], C, H, W, N_ACT),
                      D.DQNConfig(gamma=GAMMA, n_step=1, target_update_freq=FREQ, huber_delta=1.0, lr=LR))
    eager = _eager(batch)
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randint(0, 256, (batch, H, W, C), generator=g, device="cuda", dtype=torch.uint8)
    obs_next = torch.randint(0, 256, (batch, H, W, C), generator=g, device="cuda", dtype=torch.uint8)
    obs_nchw, obs_next_nchw = (x.permute(0, 3, 1, 2).contiguous() for x in (obs, obs_next))
    act = torch.randint(0, N_ACT, (batch,), generator=g, device="cuda")
    rew = torch.randn(batch, generator=g, device="cuda")
    mask = (torch.rand(batch, generator=g, device="cuda") > 0.05).float()

    def bcq_update():
        ret = rew + GAMMA * mask * bcq.target_q(obs_next)
        return bcq.update_with_batch(obs, act, ret).tolist()

    def dqn_update():
        ret = rew + GAMMA * mask * dqn.target_q(obs_next)
        return dqn.update_with_batch(obs, act, ret)[0].tolist()

    def eager_update():
        return eager(obs_nchw, obs_next_nchw, act, rew, mask)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    BI.warm_clocks()
    n, warm = max(steps, 20), max(warmup, 3)
    order = [(bcq_update, []), (dqn_update, []), (eager_update, [])]
    last = None
    for i in range(warm + n):
        k = i % 3
        for fn, sink in order[k:] + order[:k]:                      # rotate who goes first
            dt, out = timed(fn)
            if i >= warm:
                sink.append(dt)
            if fn is bcq_update:
                last = out
    sb, sd, se = (_stats(t) for _, t in order)
    return {"batch": batch, "bcq": sb, "dqn_same_inputs": sd, "eager_same_gpu": se, "timed_updates": n, "warmup": warm,
            "bcq_ms_over_dqn_ms": sb["ms_per_update_median"] / sd["ms_per_update_median"],
            "bcq_vs_eager": sb["updates_per_s_median"] / se["updates_per_s_median"],
            "bcq_not_slower_than_eager": sb["ms_per_update_median"] <= se["ms_per_update_median"],
            "final_losses": last, "parameters": bcq.P}


def run(steps: int, warmup: int) -> dict:
    big, small = run_batch(512, steps, warmup), run_batch(32, steps, warmup)
    return {
        "metric": "DiscreteBCQ engine-level updates/sec (B=512, NatureCNN trunk, two 512-wide heads, 1-step, lagged net)",
        "value": big["bcq"]["updates_per_s_median"], "unit": "updates/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic",
        "higher_is_better": True,
        "config": {"workload": f"C3-shape DiscreteBCQ: u8[84,84,4] observations, {N_ACT} actions, B=512 and B=32, 1-step, "
                               f"threshold {TAU}, penalty {THETA}, target sync every {FREQ}; one update = target pass + update",
                   "eager": "the same update on tests/standin_bcq.py modules on the same GPU, torch.optim.Adam, fp32"},
        "B512": big, "B32": small,
        "conditions": {"bcq_not_slower_than_eager": bool(big["bcq_not_slower_than_eager"] and small["bcq_not_slower_than_eager"])},
    }


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcq_bench.json"))
    a = ap.parse_args()
    res = run(a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    if not res["conditions"]["bcq_not_slower_than_eager"]:
        sys.exit("DiscreteBCQ engine is slower than the eager update")
