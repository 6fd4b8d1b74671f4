"""DQN on the dueling MLP Net at the shapes of examples/box2d/lunarlander_dqn.py and examples/discrete/discrete_dqn.py (record,
not a gate) -- the engine beside the same update in eager PyTorch on the same GPU, in one process.

    python bench_dqn_mlp.py [--steps K] [--warmup W] [--out profiles/dqn_mlp_bench.json]

One "update" = `_target_q` on the next observations with the n-step arithmetic (online and lagged network, double-Q gather) and
the update proper (forward, loss, backward, lagged copy when due, one Adam step).  The eager baseline is dqn.py:365-404 written
out below on torch.nn modules of the same shape with torch.optim.Adam.  Protocol as bench_bdqn.py: both routes timed in
alternation, each call on its own with a device synchronisation, after a clock warm-up; the figure is the median of the timed
calls.  The two halves of the engine's update are also timed on their own with device events.  No ratio is fixed in advance.
`launches_per_update` counts what the engine's route enqueues from its own code.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import copy
import json
import os
import statistics
import sys
import time

import torch
from torch import nn

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SHAPES = {       # (obs_dim, trunk, Q hidden, V hidden, actions), batch, n-step, target_update_freq: the examples' defaults
    "lunarlander_dqn": ((8, (128, 128), (128, 128), (128, 128), 4), 128, 4, 500),
    "discrete_dqn": ((4, (128, 128, 128), None, None, 2), 64, 3, 320),
}
GAMMA, LR = 0.99, 1e-3
LAUNCHES = {"target_q": 1, "update": 2, "total": 3}      # dqnm_target_kernel; dqnm_step_kernel + dqnm_apply_kernel (no gradient clipping)


class _MLP(nn.Module):
    def __init__(self, k, hidden, n_out):
        super().__init__()
        mods = []
        for h in hidden:
            mods += [nn.Linear(k, h), nn.ReLU()]
            k = h
        if n_out:
            mods.append(nn.Linear(k, n_out))
        self.model = nn.Sequential(*mods)


class EagerNet(nn.Module):
    """The module tree and forward pass of the reference's Net (utils/net/common.py:286-369)."""

    def __init__(self, layers):
        super().__init__()
        obs_dim, trunk, q, v, n_act = layers
        self.use_dueling, self.softmax, self.num_atoms = q is not None, False, 1
        self.model = _MLP(obs_dim, trunk, 0 if self.use_dueling else n_act)
        self.Q = _MLP(trunk[-1], q, n_act) if self.use_dueling else None
        self.V = _MLP(trunk[-1], v, 1) if self.use_dueling else None

    def forward(self, obs):
        h = self.model.model(obs)
        if self.use_dueling:
            q, v = self.Q.model(h), self.V.model(h)
            h = q - q.mean(dim=1, keepdim=True) + v
        return h


def _stats(times: list[float]) -> dict:
    med = statistics.median(times)
    q = statistics.quantiles(times, n=4)
    return {"updates_per_s_median": 1.0 / med, "ms_per_update_median": med * 1e3, "ms_per_update_q1": q[0] * 1e3, "ms_per_update_q3": q[2] * 1e3}


def work_per_update(layers, batch: int) -> dict:
    """Flops and bytes the algorithm needs, from the shapes: 2 K N per row and layer forward; the update runs forward, weight
    gradient and (all layers but the first) input gradient; the target pass runs two forwards.  Bytes: every parameter read once
    per forward / input-gradient pass and tile, the slabs written and read once, parameters and both moments read and written."""
    from tianshou_amd import dqn_mlp as M

    blocks = M._blocks(layers)[0]
    mac = sum(k * n for _, k, n in blocks)
    first = blocks[0][1] * blocks[0][2]
    count = M.layout(layers)["count"]
    tiles = (batch + 31) // 32
    flops = 2 * batch * (2 * mac + mac + mac + (mac - first))
    bytes_ = 4 * count * (tiles * (2 + 1 + 1) + 2 * tiles + 6)
    return {"parameters": count, "tiles": tiles, "flops": flops, "bytes": bytes_}


def bench_shape(name: str, steps: int, warmup: int) -> dict:
    import bench_init as BI
    from tianshou_amd import dqn_mlp as M
    from tianshou_amd.dqn import DQNConfig

    layers, batch, n_step, freq = SHAPES[name]
    torch.manual_seed(0)
    net = EagerNet(layers)
    assert M.describe_module(net) == layers
    cfg = DQNConfig(gamma=GAMMA, n_step=n_step, target_update_freq=freq, is_double=True, lr=LR)
    eng = M.DQNMlpEngine(layers, M.flat_from_torch([p.detach() for p in net.parameters()], *layers, "cuda"), cfg)
    net = net.cuda()
    old = copy.deepcopy(net)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    it = [0]
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randn(batch, layers[0], generator=g, device="cuda")
    obs_next = torch.randn(batch, layers[0], generator=g, device="cuda")
    act = torch.randint(0, layers[4], (batch,), generator=g, device="cuda")
    mask = (torch.rand(batch, generator=g, device="cuda") > 0.05).float()
    gpow = torch.full((batch,), GAMMA ** n_step, dtype=torch.float64, device="cuda")
    mc = torch.randn(batch, generator=g, device="cuda").double()
    rows = torch.arange(batch, device="cuda")

    def engine_update():
        loss, _ = eng.update_with_batch(obs, act, eng.target_returns(obs_next, (mask, gpow, mc)))
        return loss.item()

    def eager_update():
        with torch.no_grad():                                               # dqn.py:365-379 + algorithm_base.py:798-811
            tq = old(obs_next)[rows, net(obs_next).max(dim=1)[1]]
            ret = ((tq * mask).double() * gpow + mc).float()
        if it[0] % freq == 0:                                               # dqn.py:277-285
            old.load_state_dict(net.state_dict())
        it[0] += 1
        td = ret - net(obs)[rows, act]                                      # dqn.py:387-402
        loss = td.pow(2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item()

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
    # the engine's two calls on their own, device time between events (each includes its launches' gaps, not the host's return)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    halves = ([], [])
    for _ in range(n):
        ev[0].record()
        ret = eng.target_returns(obs_next, (mask, gpow, mc))
        ev[1].record()
        eng.update_with_batch(obs, act, ret)
        ev[2].record()
        torch.cuda.synchronize()
        halves[0].append(ev[0].elapsed_time(ev[1]) * 1e3)
        halves[1].append(ev[1].elapsed_time(ev[2]) * 1e3)
    se, sg = (_stats(t) for _, t in order)
    return {"workload": f"obs {layers[0]}, trunk {list(layers[1])}, Q {layers[2]}, V {layers[3]}, A={layers[4]}, B={batch}, n-step {n_step}, "
                        f"Adam lr {LR}, target network (freq {freq}), double",
            "engine_target_q_plus_update": se, "eager_same_gpu": sg, "engine_ms": se["ms_per_update_median"], "eager_ms": sg["ms_per_update_median"],
            "engine_vs_eager": se["updates_per_s_median"] / sg["updates_per_s_median"],
            "engine_not_slower_than_eager": se["ms_per_update_median"] <= sg["ms_per_update_median"],
            "device_us_target_q_call_median": statistics.median(halves[0]), "device_us_update_call_median": statistics.median(halves[1]),
            "first_loss_engine_eager": list(first), "timed_updates": n, "warmup": warm, **work_per_update(layers, batch)}


def run(steps: int, warmup: int) -> dict:
    shapes = {name: bench_shape(name, steps, warmup) for name in SHAPES}
    main = shapes["lunarlander_dqn"]
    return {"metric": "DQN-MLP engine-level updates/sec (lunarlander_dqn.py shape, B=128)", "value": main["engine_target_q_plus_update"]["updates_per_s_median"],
            "unit": "updates/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic", "higher_is_better": True,
            "config": {"one_update": "target_q with the n-step arithmetic on obs_next + update (step, slab sum + lagged copy + Adam)",
                       "eager": "the same target and update on torch.nn modules of the same shape on the same GPU, torch.optim.Adam, fp32"},
            "launches_per_update": LAUNCHES, "shapes": shapes}


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_mlp_bench.json"))
    a = ap.parse_args()
    res = run(a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
