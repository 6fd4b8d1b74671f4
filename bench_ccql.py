"""Continuous CQL (record, not a gate) beside SAC on the same inputs in the same process, and beside the same update in eager
PyTorch on the same GPU.

    python bench_ccql.py [--steps K] [--warmup W] [--legs L] [--eager-steps E] [--out profiles/cql_bench.json]

Shapes: examples/offline/d4rl_cql.py's (obs 17, act 6, Net[256, 256], B = 256, R = 10) and the C5 shape (obs 376, act 17,
B = 4096, R = 10).  One "update" = one engine-level `CQLEngine.update_with_batch` / `SACEngine.update_with_batch` on a batch
already on the device, noise supplied (SAC: returns supplied too -- CQL's update contains its own target pass).  Both engines start
from the same parameters and see the same batches.  A leg is `--steps` updates (five times as many at the small shape) between two device synchronisations; legs of the
two engines alternate after a clock warm-up, so that clock drift hits both alike, and the figure is the median over at least 5
legs each.  The eager figure is tests/oracle_cql.py's restatement of the reference's update on device tensors (it synchronises
where the reference does: the statistics' float() and the clip).  The stacked critic pass has 1 + 3R = 31 times SAC's critic
rows; the JSON holds the CQL : SAC time ratio beside that row ratio.  Prints one JSON line and writes it to --out.
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

SHAPES = {"d4rl_cql": (17, 6, 256), "c5": (376, 17, 4096)}
HIDDEN, R = 256, 10
LEG_SCALE = {"d4rl_cql": 5, "c5": 1}      # updates per leg = --steps times this: legs of 0.1 s and more in both shapes


def _stats(times: list[float], steps: int) -> dict:
    med = statistics.median(times)
    return {"updates_per_s_median": steps / med, "updates_per_s_min": steps / max(times), "updates_per_s_max": steps / min(times),
            "us_per_update_median": med / steps * 1e6, "legs": len(times)}


def run_shape(name: str, steps: int, warmup: int, legs: int, eager_steps: int) -> dict:
    from oracle import oracle_sac as OS
    from tests import oracle_cql as OC
    from tianshou_amd import cql as Q
    from tianshou_amd import sac as S

    obs_dim, act_dim, B = SHAPES[name]
    actor, c1, c2 = OS.init_sac_params(obs_dim, act_dim, 0, HIDDEN)
    flats = (S.actor_flat_from_torch(list(actor.values()), obs_dim, act_dim, hidden=HIDDEN),
             S.critic_flat_from_torch(list(c1.values()), obs_dim, act_dim, hidden=HIDDEN),
             S.critic_flat_from_torch(list(c2.values()), obs_dim, act_dim, hidden=HIDDEN))
    kw = dict(actor_lr=1e-4, critic_lr=3e-4, alpha_lr=1e-4, tau=0.005, auto_alpha=True, target_entropy=-float(act_dim))
    cql = Q.CQLEngine(obs_dim, act_dim, *flats, Q.CQLConfig(cql_alpha_lr=3e-4, num_repeat_actions=R, **kw), hidden=HIDDEN)
    sac = S.SACEngine(obs_dim, act_dim, *flats, S.SACConfig(**kw), hidden=HIDDEN)
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
    batches = [dict(obs=rn(B, obs_dim), act=torch.rand(B, act_dim, generator=g, device="cuda") * 2 - 1, rew=rn(B),
                    done=(torch.rand(B, generator=g, device="cuda") < 0.02).float(), obs_next=rn(B, obs_dim), noise_actor=rn(B, act_dim),
                    noise_next=rn(B, act_dim), random_act=torch.rand(B * R, act_dim, generator=g, device="cuda") * 2 - 1,
                    noise_rep_cur=rn(B * R, act_dim), noise_rep_next=rn(B * R, act_dim), calib=rn(B)) for _ in range(4)]

    def leg(which, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            b = batches[i % len(batches)]
            if which == "cql":
                stats = cql.update_with_batch(**b)
            else:
                stats, _ = sac.update_with_batch(b["obs"], b["act"], b["rew"], b["noise_actor"])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats

    for which in ("cql", "sac"):
        leg(which, max(2, warmup))
    t = {"cql": [], "sac": []}
    for i in range(legs):
        for which in (("cql", "sac") if i % 2 == 0 else ("sac", "cql")):      # alternate who goes first
            dt, stats = leg(which, steps)
            t[which].append(dt)
            if which == "cql":
                last = stats
    sc, ss = _stats(t["cql"], steps), _stats(t["sac"], steps)

    # the same update in eager PyTorch on the same GPU
    ocfg = OC.CQLConfig(cql_alpha_lr=3e-4, num_repeat_actions=R, **kw)
    dev = lambda d: {k: v.cuda() for k, v in d.items()}  # noqa: E731
    st = OC.CQLState.create(dev(actor), dev(c1), dev(c2), ocfg)
    st.cql_log_alpha, st.sac.log_alpha = st.cql_log_alpha.cuda(), st.sac.log_alpha.cuda()
    for i in range(2):
        OC.update_with_batch(st, ocfg, **batches[i % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(eager_steps):
        OC.update_with_batch(st, ocfg, **batches[i % len(batches)])
    torch.cuda.synchronize()
    eager = (time.perf_counter() - t0) / eager_steps
    ratio = sc["us_per_update_median"] / ss["us_per_update_median"]
    return {"shape": f"obs {obs_dim}, act {act_dim}, B={B}, R={R}, Net[{HIDDEN}, {HIDDEN}], AutoAlpha, Lagrange, calibrated",
            "cql": sc, "sac_same_inputs": ss, "updates_per_leg": steps, "cql_over_sac_time": ratio, "critic_rows_cql_over_sac": 1 + 3 * R,
            "eager_torch_us_per_update": eager * 1e6, "eager_torch_updates_per_s": 1.0 / eager, "eager_steps": eager_steps,
            "engine_over_eager": eager * 1e6 / sc["us_per_update_median"],
            "sac_leg_spread": (max(t["sac"]) - min(t["sac"])) / statistics.median(t["sac"]),
            "final_stats": [float(x) for x in last.tolist()]}


def run(steps: int, warmup: int, legs: int, eager_steps: int) -> dict:
    import bench_init as BI

    if not torch.cuda.is_available():
        raise RuntimeError("bench_ccql.py measures on an MI355X; there is no CPU path")
    legs = max(5, legs)
    BI.warm_clocks()
    shapes = {name: run_shape(name, steps * LEG_SCALE[name], warmup, legs, eager_steps) for name in SHAPES}
    head = shapes["d4rl_cql"]
    return {"metric": "continuous CQL engine-level updates/sec (obs 17, act 6, B=256, R=10, Net[256, 256])",
            "value": head["cql"]["updates_per_s_median"], "unit": "updates/s", "warmup": warmup, "n_gpus": 1, "dtype": "f32",
            "data": "synthetic", "higher_is_better": True, "how": "median over alternating legs after a clock warm-up; see bench_ccql.py",
            "shapes": shapes}


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", type=int, default=7)
    ap.add_argument("--eager-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cql_bench.json"))
    a = ap.parse_args()
    line = json.dumps(run(a.steps, a.warmup, a.legs, a.eager_steps))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
