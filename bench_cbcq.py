"""Continuous BCQ (record, not a gate) beside TD3 on the same rows in the same process, and beside the same update in eager
PyTorch on the same GPU.

    python bench_cbcq.py [--steps K] [--warmup W] [--legs L] [--eager-steps E] [--out profiles/cbcq_bench.json]
    python bench_cbcq.py --kernel-run d4rl_bcq      # 10 updates and nothing else, for a kernel trace of its own

Shapes: examples/offline/d4rl_bcq.py's (obs 17, act 6, Net[256, 256], VAE MLP[512, 512], L = 12, B = 256, R = 10, the plain-MLP
perturbation net) and the C5 shape (obs 376, act 17, L = 34, B = 4096, R = 10).  One "update" = one engine-level
`CBCQEngine.update_with_batch` / `TD3Engine.update_with_batch` on a batch already on the device, draws supplied (TD3: returns
supplied too -- BCQ's update contains its own target pass over B R rows).  Three engines see the same batches: BCQ with the
decoder's B (R + 1) rows in one pass, BCQ with them as two passes (`split_decode`), and TD3.  A leg is `--steps` updates (five
times as many at the small shape) between two device synchronisations; legs of the engines alternate after a clock warm-up, so
that clock drift hits all alike, and the figure is the median over at least 5 legs each.  The eager figure is
tests/oracle_cbcq.py's restatement of the reference's update on device tensors (it synchronises where the reference does: the
statistics' float() and the clip).  `policy_forward`: N = 10 observations, T = 100 candidates each in one engine call against the
oracle's per-observation loop (the reference's).  Prints one JSON line and writes it to --out.
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

SHAPES = {"d4rl_bcq": (17, 6, 256), "c5": (376, 17, 4096)}
HIDDEN, VAE_HIDDEN, R = (256, 256), (512, 512), 10
LEG_SCALE = {"d4rl_bcq": 5, "c5": 1}      # updates per leg = --steps times this: legs of 0.1 s and more in both shapes
ENGINES = ("bcq", "bcq_split", "td3")


def _stats(times: list[float], steps: int) -> dict:
    med = statistics.median(times)
    return {"updates_per_s_median": steps / med, "updates_per_s_min": steps / max(times), "updates_per_s_max": steps / min(times),
            "us_per_update_median": med / steps * 1e6, "legs": len(times)}


def _setup(name: str):
    from oracle import oracle_sac as OS
    from tests import cbcq_common as BC
    from tests import oracle_cbcq as OB
    from tianshou_amd import td3 as T

    obs_dim, act_dim, B = SHAPES[name]
    L = 2 * act_dim
    params = OB.init_params(obs_dim, act_dim, L, 0, HIDDEN, VAE_HIDDEN)
    ocfg = OB.CBCQConfig(num_sampled_action=R, pert_first_row=True, pert_lr=1e-3, critic1_lr=1e-3, critic2_lr=1e-3, vae_lr=1e-3)
    engs = {"bcq": BC.engine_from(*params, ocfg), "bcq_split": BC.engine_from(*params, ocfg, split_decode=True)}
    actor, c1, c2 = OS.init_td3_params(obs_dim, act_dim, 0)
    engs["td3"] = T.TD3Engine(obs_dim, act_dim, T.actor_flat_from_torch(list(actor.values()), obs_dim, act_dim),
                              T.critic_flat_from_torch(list(c1.values()), obs_dim, act_dim),
                              T.critic_flat_from_torch(list(c2.values()), obs_dim, act_dim), T.TD3Config())
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
    batches = [dict(obs=rn(B, obs_dim), act=torch.rand(B, act_dim, generator=g, device="cuda") * 2 - 1, rew=rn(B),
                    done=(torch.rand(B, generator=g, device="cuda") < 0.02).float(), obs_next=rn(B, obs_dim), eps1=rn(B, L),
                    eps2=rn(B * R, L), eps3=rn(B, L)) for _ in range(4)]
    return obs_dim, act_dim, B, L, params, ocfg, engs, batches


def _update(engs, which, b):
    if which == "td3":
        return engs["td3"].update_with_batch(b["obs"], b["act"], b["rew"])[0]
    return engs[which].update_with_batch(**b)


def run_shape(name: str, steps: int, warmup: int, legs: int, eager_steps: int) -> dict:
    from tests import oracle_cbcq as OB

    obs_dim, act_dim, B, L, params, ocfg, engs, batches = _setup(name)

    def leg(which, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            stats = _update(engs, which, batches[i % len(batches)])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats

    for which in ENGINES:
        leg(which, max(2, warmup))
    t = {w: [] for w in ENGINES}
    for i in range(legs):
        order = ENGINES[i % 3:] + ENGINES[:i % 3]                              # rotate who goes first
        for which in order:
            dt, stats = leg(which, steps)
            t[which].append(dt)
            if which == "bcq":
                last = stats
    s = {w: _stats(t[w], steps) for w in ENGINES}

    # the same update in eager PyTorch on the same GPU
    dev = lambda d: {k: v.cuda() for k, v in d.items()}  # noqa: E731
    st = OB.CBCQState.create(*(dev(p) for p in params), ocfg)
    for i in range(2):
        OB.update_with_batch(st, ocfg, **batches[i % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(eager_steps):
        OB.update_with_batch(st, ocfg, **batches[i % len(batches)])
    torch.cuda.synchronize()
    eager = (time.perf_counter() - t0) / eager_steps

    # policy forward: N = 10 observations, T = 100 candidates
    N, T = 10, 100
    g = torch.Generator(device="cuda").manual_seed(2)
    obs, noise = torch.randn(N, obs_dim, generator=g, device="cuda"), torch.randn(N, T, L, generator=g, device="cuda")
    eng = engs["bcq"]
    fwd_t = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            eng.policy_forward(obs, noise)
        torch.cuda.synchronize()
        fwd_t.append((time.perf_counter() - t0) / 50)
    pert, c1, _, vae = (dev(p) for p in params)
    OB.policy_forward(pert, c1, vae, ocfg, obs, noise)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        OB.policy_forward(pert, c1, vae, ocfg, obs, noise)
    torch.cuda.synchronize()
    fwd_eager = (time.perf_counter() - t0) / 5
    us = lambda w: s[w]["us_per_update_median"]  # noqa: E731
    return {"shape": f"obs {obs_dim}, act {act_dim}, L={L}, B={B}, R={R}, Net{list(HIDDEN)}, VAE MLP{list(VAE_HIDDEN)}, MLP perturbation net",
            "bcq": s["bcq"], "bcq_split_decode": s["bcq_split"], "td3_same_rows": s["td3"], "updates_per_leg": steps,
            "bcq_over_td3_time": us("bcq") / us("td3"), "merged_over_split_time": us("bcq") / us("bcq_split"),
            "eager_torch_us_per_update": eager * 1e6, "eager_torch_updates_per_s": 1.0 / eager, "eager_steps": eager_steps,
            "engine_over_eager": eager * 1e6 / us("bcq"),
            "td3_leg_spread": (max(t["td3"]) - min(t["td3"])) / statistics.median(t["td3"]),
            "policy_forward_n10_t100": {"engine_us_median": statistics.median(fwd_t) * 1e6, "eager_loop_us": fwd_eager * 1e6,
                                        "engine_over_eager": fwd_eager / statistics.median(fwd_t)},
            "final_stats": [float(x) for x in last.tolist()]}


def run(steps: int, warmup: int, legs: int, eager_steps: int) -> dict:
    import bench_init as BI

    if not torch.cuda.is_available():
        raise RuntimeError("bench_cbcq.py measures on an MI355X; there is no CPU path")
    legs = max(5, legs)
    BI.warm_clocks()
    shapes = {name: run_shape(name, steps * LEG_SCALE[name], warmup, legs, eager_steps) for name in SHAPES}
    head = shapes["d4rl_bcq"]
    return {"metric": "continuous BCQ engine-level updates/sec (obs 17, act 6, B=256, R=10, Net[256, 256], VAE MLP[512, 512])",
            "value": head["bcq"]["updates_per_s_median"], "unit": "updates/s", "warmup": warmup, "n_gpus": 1, "dtype": "f32",
            "data": "synthetic", "higher_is_better": True, "how": "median over alternating legs after a clock warm-up; see bench_cbcq.py",
            "shapes": shapes}


def kernel_run(name: str, n: int = 10) -> None:
    """`n` updates of the merged-pass engine and nothing else (no warm-up, no other engine): a kernel trace of this process
    counts n times the launches of one update."""
    *_, engs, batches = _setup(name)
    for i in range(n):
        engs["bcq"].update_with_batch(**batches[i % len(batches)])
    torch.cuda.synchronize()


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", type=int, default=7)
    ap.add_argument("--eager-steps", type=int, default=20)
    ap.add_argument("--kernel-run", default=None, choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cbcq_bench.json"))
    a = ap.parse_args()
    if a.kernel_run:
        kernel_run(a.kernel_run)
        sys.exit(0)
    line = json.dumps(run(a.steps, a.warmup, a.legs, a.eager_steps))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
