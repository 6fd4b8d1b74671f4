"""GAIL's discriminator half beside the PPO update it precedes (record, not a gate), engine level, on the networks of
examples/inverse/irl_gail.py: obs 17, act 6, all nets Net[64, 64] tanh.

    python bench_gail.py [--steps K] [--warmup W] [--legs L] [--out profiles/gail_bench.json]

Two shapes: "irl" -- N = 2048 transitions per update, disc_update_num 2 (two steps of 1024 + 1024 rows), PPO minibatch 64, repeat
10 (irl_gail.py's defaults with 2048 steps per collect); "c2" -- the C2 rollout of bench.py, N = 2^20, disc_update_num 4, PPO
minibatch 65,536, repeat 10.  Per shape, after a clock warm-up, legs of five kinds alternate in one process (the order rotates
so that clock drift hits all alike); a leg is `--steps` repetitions between two device synchronisations:
    disc_per_layer   all discriminator steps of one update, route 1 (layer by layer on the GEMM kernels)
    disc_one_launch  the same, route 2 (the one-launch kernel of ts_npg_q.h with the logistic loss)
    reward           ts_gail_reward over the whole rollout (automatic route)
    ppo_update       PPOEngine.update on the same rollout (the half GAIL inherits)
    disc_eager       the same discriminator steps in eager PyTorch on the same GPU (tests/oracle_gail.py on device tensors, the
                     per-step statistics kept on the device: kinder than the reference's three .item() per step)
The figure of a kind is the median over its legs.  Prints one JSON line and writes it to --out.
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

OBS, ACT, HIDDEN = 17, 6, [64, 64]
SHAPES = {"irl": dict(E=1, T=2048, num=2, batch=64, repeat=10, n_expert=20000),
          "c2": dict(E=512, T=2048, num=4, batch=65536, repeat=10, n_expert=1 << 20)}


def _stats(times: list[float], steps: int) -> dict:
    med = statistics.median(times)
    return {"us_median": med / steps * 1e6, "us_min": min(times) / steps * 1e6, "us_max": max(times) / steps * 1e6, "legs": len(times)}


def run_shape(name: str, steps: int, warmup: int, legs: int) -> dict:
    from oracle import oracle_ppo as OP
    from tests import oracle_gail as OG
    from tianshou_amd import gail as G
    from tianshou_amd import ppo as P
    from tianshou_amd.buffer import random_permutation

    s = SHAPES[name]
    n = s["E"] * s["T"]
    g = torch.Generator(device="cuda").manual_seed(3)
    obs = torch.randn(n + 1, OBS, generator=g, device="cuda")
    act = torch.randn(n, ACT, generator=g, device="cuda")
    e_obs = torch.randn(s["n_expert"], OBS, generator=g, device="cuda") + 0.4
    e_act = torch.tanh(torch.randn(s["n_expert"], ACT, generator=g, device="cuda"))
    term = torch.rand(n, generator=g, device="cuda") < 0.01
    trunc = torch.zeros(n, dtype=torch.bool, device="cuda")
    cut = torch.arange(s["E"], device="cuda") * s["T"] + s["T"] - 1
    bsz, n_steps = G.chunking(n, s["num"])
    t0 = OG.init_disc(OBS + ACT, HIDDEN, 5)
    flat = G.GAILDiscriminator.flat_from_tensors(t0, OBS, ACT, HIDDEN)
    mk = lambda route: G.GAILDiscriminator(OBS, ACT, HIDDEN, "tanh", flat, e_obs, e_act,                       # noqa: E731
                                           G.GAILConfig(disc_update_num=s["num"], lr=2.5e-5, route=route))
    engs = {"disc_per_layer": mk("per_layer"), "disc_one_launch": mk("one_launch"), "reward": mk("auto")}
    ppo = P.PPOEngine(OBS, ACT, OP.flatten_params(OP.init_params(OBS, ACT, seed=1)).cuda(),
                      P.PPOConfig(lr=3e-4, max_grad_norm=0.5, vf_coef=0.25, ent_coef=0.001))
    perm = random_permutation(n, 11, "cuda")
    ei = torch.randint(0, s["n_expert"], (n_steps * bsz,), generator=g, device="cuda")
    rew = engs["reward"].reward(obs[:n], act)
    b = ppo.preprocess(obs[:n], obs[1:], act, rew, term, trunc, cut)
    perms = [random_permutation(n, 100 + r, "cuda") for r in range(s["repeat"])]
    eager = {"t": [x.cuda() for x in t0], "opt": OG.Adam(lr=2.5e-5)}

    def op(kind):
        if kind == "reward":
            return engs[kind].reward(obs[:n], act)
        if kind == "ppo_update":
            return ppo.update(b, s["batch"], s["repeat"], perms)
        if kind == "disc_eager":
            eager["t"], st = OG.disc_update(eager["t"], eager["opt"], obs[:n], act, perm, e_obs, e_act, ei, s["num"], "tanh")
            return st
        return engs[kind].disc_update(obs[:n], act, perm, ei)

    def leg(kind, k):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(k):
            out = op(kind)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    kinds = ["disc_per_layer", "disc_one_launch", "reward", "ppo_update", "disc_eager"]
    for kind in kinds:
        leg(kind, max(1, warmup))
    times = {k: [] for k in kinds}
    last = {}
    for i in range(legs):
        for kind in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:          # rotate who goes first
            dt, out = leg(kind, steps)
            times[kind].append(dt)
            last[kind] = out
    res = {k: _stats(v, steps) for k, v in times.items()}
    res["config"] = dict(N=n, disc_update_num=s["num"], bsz=bsz, disc_steps=n_steps, ppo_minibatch=s["batch"], ppo_repeat=s["repeat"],
                         ppo_gradient_steps=int(last["ppo_update"][1]), expert_rows=s["n_expert"])
    res["one_launch_over_per_layer"] = res["disc_one_launch"]["us_median"] / res["disc_per_layer"]["us_median"]
    res["eager_over_per_layer"] = res["disc_eager"]["us_median"] / res["disc_per_layer"]["us_median"]
    res["eager_over_one_launch"] = res["disc_eager"]["us_median"] / res["disc_one_launch"]["us_median"]
    res["disc_over_ppo_update"] = min(res["disc_one_launch"]["us_median"], res["disc_per_layer"]["us_median"]) / res["ppo_update"]["us_median"]
    res["last_disc_stats"] = {k: [float(x) for x in last[k][-1].tolist()] for k in ("disc_per_layer", "disc_one_launch", "disc_eager")}
    return res


def run(steps: int, warmup: int, legs: int) -> dict:
    import bench_init as BI

    if not torch.cuda.is_available():
        raise RuntimeError("bench_gail.py measures on an MI355X; there is no CPU path")
    legs = max(5, legs)
    BI.warm_clocks()
    irl = run_shape("irl", steps, warmup, legs)
    BI.warm_clocks()
    c2 = run_shape("c2", max(1, steps // 10), max(1, warmup // 10), legs)
    best = min(irl["disc_per_layer"]["us_median"], irl["disc_one_launch"]["us_median"])
    return {"metric": "GAIL discriminator phase per update, engine level (obs 17, act 6, Net[64, 64] tanh, N=2048, disc_update_num 2)",
            "value": best, "unit": "us/update", "higher_is_better": False, "n_gpus": 1, "dtype": "f32", "data": "synthetic",
            "steps_per_leg": {"irl": steps, "c2": max(1, steps // 10)}, "warmup": warmup, "irl": irl, "c2": c2}


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--legs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gail_bench.json"))
    a = ap.parse_args()
    line = json.dumps(run(a.steps, a.warmup, a.legs))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
