"""FQF on the plain MLP Net at the shape of test/discrete/test_fqf.py (record, not a gate) -- the engine beside the same update in
eager PyTorch on the same GPU and beside the IQN-MLP engine at the same trunk and N, in one process.

    python bench_fqf_mlp.py [--steps K] [--warmup W] [--out profiles/fqf_mlp_bench.json]

One "update" = `_target_q` on the next observations with the n-step arithmetic on the [B, N] target (the online network proposes the
fractions and selects, the lagged network is walked over the same fractions) and the update proper (proposal, forward at tau_hats
and at the interior taus, quantile Huber loss, fraction and entropy loss, both backward passes, lagged copy when due, Adam on the
model, RMSprop on the fraction network).  The eager baseline is fqf.py:66-106, 178-256 and discrete.py:239-314 written out below
on torch.nn modules of the same shape with torch.optim.  The IQN-MLP leg is bench_iqn_mlp.py's update on the same trunk with N
drawn fractions; its `last` stops at two hidden layers (its envelope), so at test_fqf.py's shape it runs one layer less, and the
second shape (no hidden layer in `last`) gives both engines the same network.
Protocol: bench_iqn_mlp.py's (clock warm-up, 7 alternating legs of K updates, each update on its own with a device synchronisation,
median of the legs' medians, spread = their minimum and maximum).  No ratio is fixed in advance.  Prints one JSON line and writes
it to --out.
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

SHAPES = {       # (obs_dim, trunk, linear feature width, cosines, `last` hidden, actions), fractions N, batch, n-step, target_update_freq
    "test_fqf": ((4, (64, 64), 64, 64, (64, 64, 64), 2), 32, 64, 3, 320),
    "test_fqf_head_only": ((4, (64, 64), 64, 64, (), 2), 32, 64, 3, 320),
}
GAMMA, LR, F_LR, ENT_COEF, LEGS = 0.9, 1e-3, 2.5e-9, 10.0, 7           # test_fqf.py: fraction_lr 2.5e-9, ent_coef 10
LAUNCHES = {"next_dist": 1, "update": 3, "total": 4}       # fqfm_walk_kernel; fqfm_step_kernel + fqfm_apply_kernel + the fraction optimizer


def quantiles(net, f, taus):
    """FullQuantileFunction._compute_quantiles (discrete.py:288-291) with CosineEmbeddingNetwork.forward (:144-160)."""
    b, n = taus.shape
    i_pi = math.pi * torch.arange(1, net.n_cos + 1, dtype=f.dtype, device=f.device).view(1, 1, -1)
    emb = net.embed_model.net(torch.cos(taus.unsqueeze(2) * i_pi).view(-1, net.n_cos)).view(b, n, -1)
    return net.last.model((f.unsqueeze(1) * emb).view(b * n, -1)).view(b, n, -1).transpose(1, 2)


def eager_forward(net, frac, obs, fractions=None, want_tau=False):
    """FullQuantileFunction.forward + FractionProposalNetwork.forward + FQFPolicy.forward's weighted arg-max."""
    f = net.preprocess.model.model(obs)
    if fractions is None:
        dist = torch.distributions.Categorical(logits=frac.net(f.detach()))
        taus = nn.functional.pad(torch.cumsum(dist.probs, dim=1), (1, 0))
        fractions = (taus, (taus[:, :-1] + taus[:, 1:]).detach() / 2.0, dist.entropy())
    taus, tau_hats, _ = fractions
    logits = quantiles(net, f, tau_hats)
    with torch.no_grad():
        q_tau = quantiles(net, f, taus[:, 1:-1]) if want_tau else None
        act = ((taus[:, 1:] - taus[:, :-1]).unsqueeze(1) * logits).sum(2).max(dim=1)[1]
    return logits, fractions, q_tau, act


def bench_shape(name: str, steps: int, warmup: int) -> dict:
    import bench_init as BI
    from bench_iqn_mlp import EagerIQN
    from tianshou_amd import fqf_mlp as M
    from tianshou_amd import iqn_mlp as I
    from tianshou_amd.iqn import IQNConfig

    layers, n, batch, n_step, freq = SHAPES[name]
    torch.manual_seed(0)
    net, frac = EagerIQN(layers), nn.Module()
    frac.net = nn.Linear(layers[2], n)
    nn.init.xavier_uniform_(frac.net.weight, gain=0.01)
    nn.init.constant_(frac.net.bias, 0)
    assert M.describe_module(net, frac) == (layers, n)
    cfg = M.FQFConfig(gamma=GAMMA, n_step=n_step, target_update_freq=freq, ent_coef=ENT_COEF, lr=LR, f_optimizer="rmsprop", f_lr=F_LR)
    eng = M.FQFMlpEngine(layers, n, M.flat_from_torch([p.detach() for p in net.parameters()], *layers, "cuda"),
                         M.fraction_from_torch([p.detach() for p in frac.parameters()], layers[2], n, "cuda"), cfg)
    ilayers = layers[:4] + (layers[4][:I.MAX_LAST],) + layers[5:]
    inet = EagerIQN(ilayers)
    ieng = I.IQNMlpEngine(ilayers, I.flat_from_torch([p.detach() for p in inet.parameters()], *ilayers, "cuda"),
                          IQNConfig(n_cos=layers[3], online_sample_size=n, target_sample_size=n, gamma=GAMMA, n_step=n_step,
                                    target_update_freq=freq, lr=LR))
    net, frac = net.cuda(), frac.cuda()
    old = copy.deepcopy(net)
    opt, f_opt = torch.optim.Adam(net.parameters(), lr=LR), torch.optim.RMSprop(frac.parameters(), lr=F_LR)
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
        losses, _ = eng.update_with_batch(obs, act, eng.target_returns(obs_next, (mask, gpow, mc)))
        return losses.tolist()

    def iqn_update():
        loss, _ = ieng.update_with_batch(obs, act, ieng.target_returns(obs_next, (mask, gpow, mc)))
        return loss.item()

    def eager_update():
        with torch.no_grad():                                               # fqf.py:178-193 + algorithm_base.py:798-811
            _, fr, _, a = eager_forward(net, frac, obs_next)
            td = eager_forward(old, frac, obs_next, fractions=fr)[0][rows, a]
            ret = ((td * mask.view(-1, 1)).double() * gpow.view(-1, 1) + mc.view(-1, 1)).float()
        if it[0] % freq == 0:                                               # dqn.py:277-285
            old.load_state_dict(net.state_dict())
        it[0] += 1
        lg, (taus, tau_hats, ent), q_tau, _ = eager_forward(net, frac, obs, want_tau=True)      # fqf.py:200-247
        curr = lg[rows, act].unsqueeze(2)
        target = ret.unsqueeze(1)
        diff = nn.functional.smooth_l1_loss(target.expand(-1, curr.shape[1], -1), curr.expand(-1, -1, target.shape[2]), reduction="none")
        quantile_loss = (diff * (tau_hats.unsqueeze(2) - (target - curr).detach().le(0.0).float()).abs()).sum(-1).mean(1).mean()
        prio = diff.detach().abs().sum(-1).mean(1)                          # fqf.py:220  # noqa: F841
        with torch.no_grad():
            hat, th = lg[rows, act], q_tau[rows, act]
            v1, v2 = th - hat[:, :-1], th - hat[:, 1:]
            s1 = th > torch.cat([hat[:, :1], th[:, :-1]], dim=1)
            s2 = th < torch.cat([th[:, 1:], hat[:, -1:]], dim=1)
            grad_taus = torch.where(s1, v1, -v1) + torch.where(s2, v2, -v2)
        fraction_loss = (grad_taus * taus[:, 1:-1]).sum(1).mean()
        entropy_loss = ent.mean()
        f_opt.zero_grad()
        (fraction_loss - ENT_COEF * entropy_loss).backward(retain_graph=True)
        f_opt.step()
        opt.zero_grad()
        quantile_loss.backward()
        opt.step()
        return quantile_loss.item(), fraction_loss.item(), entropy_loss.item()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    BI.warm_clocks()
    k_upd, warm = max(steps, 20), max(warmup, 3)
    routes = [(engine_update, []), (eager_update, []), (iqn_update, [])]
    for fn, _ in routes:
        for _ in range(warm):
            fn()
    for leg in range(LEGS):
        k = leg % len(routes)
        for fn, sink in routes[k:] + routes[:k]:                            # alternate who goes first
            sink.append(statistics.median(timed(fn)[0] for _ in range(k_upd)))

    def stats(legs):
        return {"ms_per_update_median": statistics.median(legs) * 1e3, "ms_per_update_min_leg": min(legs) * 1e3, "ms_per_update_max_leg": max(legs) * 1e3}

    se, sg, si = (stats(t) for _, t in routes)
    lay = M.layout(layers, n, batch)
    return {"workload": f"obs {layers[0]}, Net {list(layers[1])} -> {layers[2]}, C={layers[3]}, last hidden {list(layers[4])}, A={layers[5]}, "
                        f"N={n}, B={batch}, n-step {n_step}, Adam lr {LR}, RMSprop lr {F_LR} on the fraction network, ent_coef {ENT_COEF}, "
                        f"target network (freq {freq})",
            "engine_next_dist_plus_update": se, "eager_same_gpu": sg, "iqn_mlp_engine_same_process": si,
            "iqn_mlp_last_hidden": list(ilayers[4]),
            "engine_ms": se["ms_per_update_median"], "eager_ms": sg["ms_per_update_median"], "iqn_mlp_ms": si["ms_per_update_median"],
            "engine_vs_eager": sg["ms_per_update_median"] / se["ms_per_update_median"],
            "engine_not_slower_than_eager": se["ms_per_update_max_leg"] <= sg["ms_per_update_min_leg"],
            "legs": LEGS, "timed_updates_per_leg": k_upd, "warmup": warm, "parameters": eng.P, "fraction_parameters": eng.P2,
            "tiles": (batch + 31) // 32, "lds_bytes_per_tile": lay["lds_bytes"]}


def run(steps: int, warmup: int) -> dict:
    shapes = {name: bench_shape(name, steps, warmup) for name in SHAPES}
    main = shapes["test_fqf"]
    return {"metric": "FQF-MLP engine-level updates/sec (test_fqf.py shape, B=64)", "value": 1e3 / main["engine_ms"],
            "unit": "updates/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic", "higher_is_better": True,
            "config": {"one_update": "next_dist with the n-step arithmetic on obs_next + update (step, slab sums + lagged copy + Adam, RMSprop on the "
                                     "fraction network); the fractions are proposed inside the kernels",
                       "eager": "the same target and update on torch.nn modules of the same shape on the same GPU, torch.optim, fp32",
                       "iqn_mlp": "the IQN-MLP engine's target + update on the same trunk with N drawn fractions (`last` cut to its two-layer envelope)"},
            "launches_per_update": LAUNCHES, "shapes": shapes}


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fqf_mlp_bench.json"))
    a = ap.parse_args()
    res = run(a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
