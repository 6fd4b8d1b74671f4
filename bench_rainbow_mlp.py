"""Rainbow on the dueling noisy MLP Net at the shape of test/discrete/test_rainbow.py and at LunarLander's spaces (record, not a gate) --
the engine beside the same update in eager PyTorch and beside C51MlpEngine on the same trunk, actions and atoms, on the same GPU, in one
process.

    python bench_rainbow_mlp.py [--steps K] [--warmup W] [--out profiles/rainbow_mlp_bench.json]

One "update" = `_update_with_batch` on given n-step returns of the support, both networks' noise already drawn: the periodic sync,
`_target_dist` on the next observations, forward, cross-entropy, backward, one Adam step.  The eager baseline is rainbow.py / c51.py
written out below on torch.nn modules of the same shape (NoisyLinear.forward as utils/net/discrete.py:366-374) with torch.optim.Adam; the
C51 route is bench_c51_mlp.py's engine (no dueling, no noise).  Protocol: after a clock warm-up the three routes run in 7 alternating legs
of K updates each, every update on its own with a device synchronisation; a leg's figure is the median of its updates, the reported figure
the median of the 7 legs, the spread their minimum and maximum.  No ratio is fixed in advance.  Prints one JSON line and writes it to --out.
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

SHAPES = {       # (obs_dim, trunk, Q hidden, V hidden, actions, atoms, noisy), batch, n-step, target_update_freq
    "test_rainbow": ((4, (128,) * 4, (), (), 2, 51, True), 64, 3, 320),
    "lunarlander": ((8, (128,) * 4, (), (), 4, 51, True), 128, 3, 320),
}
GAMMA, LR, LEGS, V_MIN, V_MAX, NOISY_STD = 0.9, 1e-3, 7, -10.0, 10.0, 0.1
LAUNCHES = {"update": 2, "total": 2}      # rbm_kernel<STEP> (target distribution included) + dqnm_apply_kernel (no gradient clipping)


class NoisyLinear(nn.Module):
    """utils/net/discrete.py:317-374, the noise given."""

    def __init__(self, k, n, std):
        super().__init__()
        self.mu_W = nn.Parameter(torch.empty(n, k).uniform_(-k ** -0.5, k ** -0.5))
        self.sigma_W = nn.Parameter(torch.full((n, k), std * k ** -0.5))
        self.mu_bias = nn.Parameter(torch.empty(n).uniform_(-k ** -0.5, k ** -0.5))
        self.sigma_bias = nn.Parameter(torch.full((n,), std * k ** -0.5))
        f = lambda m: (lambda x: x.sign() * x.abs().sqrt())(torch.randn(m))  # noqa: E731
        self.eps_p, self.eps_q = nn.Parameter(f(k), requires_grad=False), nn.Parameter(f(n), requires_grad=False)
        self.in_features, self.out_features = k, n

    def forward(self, x):
        return nn.functional.linear(x, self.mu_W + self.sigma_W * self.eps_q.ger(self.eps_p), self.mu_bias + self.sigma_bias * self.eps_q.clone())


class EagerNet(nn.Module):
    """The module tree and forward pass of the reference's Net (utils/net/common.py:286-369) with softmax=True, num_atoms and noisy streams."""

    def __init__(self, layers):
        super().__init__()
        obs_dim, trunk, _, _, n_act, n_atoms, _ = layers
        self.use_dueling, self.softmax, self.num_atoms = True, True, n_atoms
        mods, k = [], obs_dim
        for h in trunk:
            mods += [nn.Linear(k, h), nn.ReLU()]
            k = h
        self.model, self.Q, self.V = nn.Module(), nn.Module(), nn.Module()
        self.model.model = nn.Sequential(*mods)
        self.Q.model, self.V.model = nn.Sequential(NoisyLinear(k, n_act * n_atoms, NOISY_STD)), nn.Sequential(NoisyLinear(k, n_atoms, NOISY_STD))

    def forward(self, obs):
        h = self.model.model(obs)
        q, v = self.Q.model(h).view(obs.shape[0], -1, self.num_atoms), self.V.model(h).view(obs.shape[0], -1, self.num_atoms)
        return torch.softmax(q - q.mean(dim=1, keepdim=True) + v, dim=-1)


def bench_shape(name: str, steps: int, warmup: int) -> dict:
    import bench_init as BI
    from tianshou_amd import c51_mlp as C5
    from tianshou_amd import rainbow_mlp as M
    from tianshou_amd.dqn import DQNConfig

    layers, batch, n_step, freq = SHAPES[name]
    torch.manual_seed(0)
    net = EagerNet(layers)
    assert M.describe_module(net) == layers
    cfg = DQNConfig(gamma=GAMMA, n_step=n_step, target_update_freq=freq, lr=LR)
    sd = net.state_dict()
    noise = M.noise_from_torch([sd[k] for k in M.noise_keys(layers)], *layers, "cuda")
    eng = M.RainbowMlpEngine(layers, M.flat_from_torch([sd[k] for k in M.state_dict_keys(layers)], *layers, "cuda"), noise, cfg, v_min=V_MIN, v_max=V_MAX)
    c51_layers = (layers[0], layers[1], layers[4], layers[5])
    c51 = C5.C51MlpEngine(c51_layers, torch.randn(C5.layout(c51_layers)["count"], device="cuda") * 0.05, cfg, v_min=V_MIN, v_max=V_MAX)
    net = net.cuda()
    old = copy.deepcopy(net)
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=LR)
    it = [0]
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randn(batch, layers[0], generator=g, device="cuda")
    obs_next = torch.randn(batch, layers[0], generator=g, device="cuda")
    act = torch.randint(0, layers[4], (batch,), generator=g, device="cuda")
    mask = (torch.rand(batch, generator=g, device="cuda") > 0.05).float()
    mc = 3 * torch.randn(batch, generator=g, device="cuda").double()
    z, dz = eng.support, eng.delta_z
    ret = ((z.view(1, -1) * mask.view(-1, 1)).double() * GAMMA ** n_step + mc.view(-1, 1)).float()     # algorithm_base.py:798-811 on the support
    rows = torch.arange(batch, device="cuda")

    def engine_update():
        return eng.update_with_batch(obs, act, obs_next, ret)[0].item()

    def c51_update():
        return c51.update_with_batch(obs, act, obs_next, ret)[0].item()

    def eager_update():
        if it[0] % freq == 0:                                               # dqn.py:277-285, before the target (c51.py:147)
            old.load_state_dict(net.state_dict())
        it[0] += 1
        with torch.no_grad():                                               # c51.py:123-141
            nd = old(obs_next)[rows, (net(obs_next) * z).sum(2).max(dim=1)[1]]
            ts = ret.clamp(V_MIN, V_MAX)
            target = ((1 - (ts.unsqueeze(1) - z.view(1, -1, 1)).abs() / dz).clamp(0, 1) * nd.unsqueeze(1)).sum(-1)
        ce = -(target * torch.log(net(obs)[rows, act] + 1e-8)).sum(1)       # c51.py:151-157
        loss = ce.mean()
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

    first = (timed(engine_update)[1], timed(eager_update)[1])                # the same parameters, noise and batch: the same loss
    BI.warm_clocks()
    n, warm = max(steps, 20), max(warmup, 3)
    routes = [(engine_update, []), (eager_update, []), (c51_update, [])]
    for fn, _ in routes:
        for _ in range(warm):
            fn()
    for leg in range(LEGS):
        k = leg % 3
        for fn, sink in routes[k:] + routes[:k]:                            # alternate who goes first
            sink.append(statistics.median(timed(fn)[0] for _ in range(n)))

    def stats(legs):
        return {"ms_per_update_median": statistics.median(legs) * 1e3, "ms_per_update_min_leg": min(legs) * 1e3, "ms_per_update_max_leg": max(legs) * 1e3}

    se, sg, sc = (stats(t) for _, t in routes)
    return {"workload": f"obs {layers[0]}, trunk {list(layers[1])}, noisy dueling streams without hidden layers (noisy_std {NOISY_STD}), A={layers[4]}, "
                        f"N={layers[5]}, B={batch}, n-step {n_step}, Adam lr {LR}, target network (freq {freq}), support [{V_MIN}, {V_MAX}]",
            "engine_update": se, "eager_same_gpu": sg, "c51_mlp_engine_same_trunk": sc, "engine_ms": se["ms_per_update_median"],
            "eager_ms": sg["ms_per_update_median"], "c51_mlp_ms": sc["ms_per_update_median"],
            "engine_vs_eager": sg["ms_per_update_median"] / se["ms_per_update_median"],
            "engine_vs_c51_mlp": se["ms_per_update_median"] / sc["ms_per_update_median"],
            "engine_not_slower_than_eager": se["ms_per_update_max_leg"] <= sg["ms_per_update_min_leg"],
            "first_loss_engine_eager": list(first), "legs": LEGS, "timed_updates_per_leg": n, "warmup": warm,
            "parameters": eng.P, "tiles": (batch + 31) // 32, "lds_bytes_per_tile": M.layout(layers, batch)["lds_bytes"]}


def run(steps: int, warmup: int) -> dict:
    shapes = {name: bench_shape(name, steps, warmup) for name in SHAPES}
    main = shapes["test_rainbow"]
    return {"metric": "Rainbow-MLP engine-level updates/sec (test_rainbow.py shape, B=64)", "value": 1e3 / main["engine_ms"],
            "unit": "updates/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic", "higher_is_better": True,
            "config": {"one_update": "update_with_batch on given support returns and noise (step with the target distribution inside, slab sum + lagged copy + Adam)",
                       "eager": "the same target and update on torch.nn modules of the same shape on the same GPU, torch.optim.Adam, fp32",
                       "c51_mlp": "C51MlpEngine.update_with_batch on the same trunk, actions, atoms and batch"},
            "launches_per_update": LAUNCHES, "shapes": shapes}


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rainbow_mlp_bench.json"))
    a = ap.parse_args()
    res = run(a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
