"""IQN on the plain MLP Net at the shape of test/discrete/test_iqn.py and at LunarLander's spaces (record, not a gate) -- the engine
beside the same update in eager PyTorch on the same GPU and beside the QRDQN-MLP engine, in one process.

    python bench_iqn_mlp.py [--steps K] [--warmup W] [--out profiles/iqn_mlp_bench.json]

One "update" = `_target_q` on the next observations with the n-step arithmetic on the [B, N'] target (online and lagged network)
and the update proper (forward over the N sampled fractions, quantile Huber loss, backward, lagged copy when due, one Adam step);
the fractions are drawn per call on both routes (the engine's Philox stream, torch.rand).  The eager baseline is qrdqn.py:94-106 and
iqn.py:156-183 written out below on torch.nn modules of the same shape with torch.optim.Adam.  The QRDQN-MLP leg is
bench_qrdqn_mlp.py's update on a Net with the same trunk and N quantiles per action: the sibling route on the same tile.
Protocol: after a clock warm-up the routes run in 7 alternating legs of K updates each, every update on its own with a device
synchronisation; a leg's figure is the median of its updates, the reported figure the median of the 7 legs, the spread their
minimum and maximum.  No ratio is fixed in advance.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import copy
import json
import math
import os
import statistics
import sys
import time

import torch
from torch import nn

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SHAPES = {       # (obs_dim, trunk, linear feature width, cosines, `last` hidden, actions), samples N = N', batch, n-step, target_update_freq
    "test_iqn": ((4, (64, 64), 64, 64, (), 2), 8, 64, 3, 320),
    "lunarlander": ((8, (128, 128), 128, 64, (), 4), 8, 128, 3, 320),
}
GAMMA, LR, LEGS = 0.9, 1e-3, 7
LAUNCHES = {"next_dist": 1, "update": 2, "total": 3, "fraction_draws": 3}      # iqnm_walk_kernel; iqnm_step_kernel + dqnm_apply_kernel


def mlp(k, widths, out):
    mods = []
    for h in widths:
        mods += [nn.Linear(k, h), nn.ReLU()]
        k = h
    m = nn.Module()
    m.model = nn.Sequential(*mods, *([nn.Linear(k, out)] if out else []))
    return m


class EagerIQN(nn.Module):
    """The module tree and forward pass of ImplicitQuantileNetwork on a Net (utils/net/discrete.py:126-216, common.py:286-369)."""

    def __init__(self, layers):
        super().__init__()
        obs_dim, trunk, feat, n_cos, hidden, n_act = layers
        self.preprocess = nn.Module()
        self.preprocess.model = mlp(obs_dim, trunk, feat)
        self.preprocess.use_dueling, self.preprocess.softmax, self.preprocess.num_atoms = False, False, 1
        self.last = mlp(feat or trunk[-1], hidden, n_act)
        self.embed_model = nn.Module()
        self.embed_model.net = nn.Sequential(nn.Linear(n_cos, feat or trunk[-1]), nn.ReLU())
        self.n_cos = n_cos

    def forward(self, obs, n):
        f = self.preprocess.model.model(obs)
        taus = torch.rand(obs.shape[0], n, dtype=f.dtype, device=f.device)
        i_pi = math.pi * torch.arange(1, self.n_cos + 1, dtype=f.dtype, device=f.device).view(1, 1, -1)
        emb = self.embed_model.net(torch.cos(taus.unsqueeze(2) * i_pi).view(-1, self.n_cos)).view(obs.shape[0], n, -1)
        out = self.last.model((f.unsqueeze(1) * emb).view(obs.shape[0] * n, -1)).view(obs.shape[0], n, -1).transpose(1, 2)
        return out, taus


def bench_shape(name: str, steps: int, warmup: int) -> dict:
    import bench_init as BI
    import bench_qrdqn_mlp as BQ
    from tianshou_amd import iqn_mlp as M
    from tianshou_amd import qrdqn_mlp as Q
    from tianshou_amd.dqn import DQNConfig
    from tianshou_amd.iqn import IQNConfig

    layers, n, batch, n_step, freq = SHAPES[name]
    torch.manual_seed(0)
    net = EagerIQN(layers)
    assert M.describe_module(net) == layers
    cfg = IQNConfig(n_cos=layers[3], online_sample_size=n, target_sample_size=n, gamma=GAMMA, n_step=n_step, target_update_freq=freq, lr=LR)
    eng = M.IQNMlpEngine(layers, M.flat_from_torch([p.detach() for p in net.parameters()], *layers, "cuda"), cfg)
    qlayers = (layers[0], layers[1], layers[5], n)
    qnet = BQ.EagerNet(qlayers)
    qeng = Q.QRDQNMlpEngine(qlayers, Q.flat_from_torch([p.detach() for p in qnet.parameters()], *qlayers, "cuda"),
                            DQNConfig(gamma=GAMMA, n_step=n_step, target_update_freq=freq, is_double=True, lr=LR))
    net = net.cuda()
    old = copy.deepcopy(net)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    it = [0]
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randn(batch, layers[0], generator=g, device="cuda")
    obs_next = torch.randn(batch, layers[0], generator=g, device="cuda")
    act = torch.randint(0, layers[5], (batch,), generator=g, device="cuda")
    mask = (torch.rand(batch, generator=g, device="cuda") > 0.05).float()
    gpow = torch.full((batch,), GAMMA ** n_step, dtype=torch.float64, device="cuda")
    mc = torch.randn(batch, generator=g, device="cuda").double()
    rows = torch.arange(batch, device="cuda")

    def engine_update():
        loss, _ = eng.update_with_batch(obs, act, eng.target_returns(obs_next, (mask, gpow, mc)))
        return loss.item()

    def qrdqn_update():
        loss, _ = qeng.update_with_batch(obs, act, qeng.target_returns(obs_next, (mask, gpow, mc)))
        return loss.item()

    def eager_update():
        with torch.no_grad():                                               # qrdqn.py:94-106 + algorithm_base.py:798-811
            a = net(obs_next, n)[0].mean(2).max(dim=1)[1]
            td = old(obs_next, n)[0][rows, a]
            ret = ((td * mask.view(-1, 1)).double() * gpow.view(-1, 1) + mc.view(-1, 1)).float()
        if it[0] % freq == 0:                                               # dqn.py:277-285
            old.load_state_dict(net.state_dict())
        it[0] += 1
        lg, taus = net(obs, n)                                              # iqn.py:162-180
        curr = lg[rows, act].unsqueeze(2)
        target = ret.unsqueeze(1)
        diff = nn.functional.smooth_l1_loss(target.expand(-1, curr.shape[1], -1), curr.expand(-1, -1, target.shape[2]), reduction="none")
        loss = (diff * (taus.unsqueeze(2) - (target - curr).detach().le(0.0).float()).abs()).sum(-1).mean(1).mean()
        prio = diff.detach().abs().sum(-1).mean(1)                          # iqn.py:180  # noqa: F841
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

    BI.warm_clocks()
    k_upd, warm = max(steps, 20), max(warmup, 3)
    routes = [(engine_update, []), (eager_update, []), (qrdqn_update, [])]
    for fn, _ in routes:
        for _ in range(warm):
            fn()
    for leg in range(LEGS):
        k = leg % len(routes)
        for fn, sink in routes[k:] + routes[:k]:                            # alternate who goes first
            sink.append(statistics.median(timed(fn)[0] for _ in range(k_upd)))

    def stats(legs):
        return {"ms_per_update_median": statistics.median(legs) * 1e3, "ms_per_update_min_leg": min(legs) * 1e3, "ms_per_update_max_leg": max(legs) * 1e3}

    se, sg, sq = (stats(t) for _, t in routes)
    return {"workload": f"obs {layers[0]}, Net {list(layers[1])} -> {layers[2]}, C={layers[3]}, last hidden {list(layers[4])}, A={layers[5]}, "
                        f"N=N'={n}, B={batch}, n-step {n_step}, Adam lr {LR}, target network (freq {freq})",
            "engine_next_dist_plus_update": se, "eager_same_gpu": sg, "qrdqn_mlp_engine_same_process": sq,
            "engine_ms": se["ms_per_update_median"], "eager_ms": sg["ms_per_update_median"], "qrdqn_mlp_ms": sq["ms_per_update_median"],
            "engine_vs_eager": sg["ms_per_update_median"] / se["ms_per_update_median"],
            "engine_not_slower_than_eager": se["ms_per_update_max_leg"] <= sg["ms_per_update_min_leg"],
            "legs": LEGS, "timed_updates_per_leg": k_upd, "warmup": warm, "parameters": eng.P, "tiles": (batch + 31) // 32,
            "lds_bytes_per_tile": M.layout(layers)["lds_bytes"]}


def run(steps: int, warmup: int) -> dict:
    shapes = {name: bench_shape(name, steps, warmup) for name in SHAPES}
    main = shapes["test_iqn"]
    return {"metric": "IQN-MLP engine-level updates/sec (test_iqn.py shape, B=64)", "value": 1e3 / main["engine_ms"],
            "unit": "updates/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic", "higher_is_better": True,
            "config": {"one_update": "next_dist with the n-step arithmetic on obs_next + update (step, slab sum + lagged copy + Adam), fractions drawn per call",
                       "eager": "the same target and update on torch.nn modules of the same shape on the same GPU, torch.optim.Adam, fp32",
                       "qrdqn_mlp": "the QRDQN-MLP engine's target + update on a Net with the same trunk and N quantiles per action"},
            "launches_per_update": LAUNCHES, "shapes": shapes}


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iqn_mlp_bench.json"))
    a = ap.parse_args()
    res = run(a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
