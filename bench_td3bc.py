"""TD3+BC on the C5 shape (record, not a gate): obs 376, act 17, B = 4096, Net[256, 256] -- beside TD3 on the same inputs in the
same process.

    python bench_td3bc.py [--steps K] [--warmup W] [--legs L] [--out profiles/td3bc_bench.json]

One "update" = one engine-level `update_with_batch` on a batch already on the device with returns supplied (critic steps; on
every second update the actor step and the Polyak updates): the part of TD3BC.update() in which TD3+BC differs from TD3.  The two
engines (TD3BCEngine, TD3Engine) start from the same parameters and see the same batches.  A leg is `--steps` updates between two
device synchronisations; legs of the two engines alternate after a clock warm-up, so that clock drift hits both alike, and the
figure is the median over at least 5 legs each.  The expectation is a ratio of 1: TD3+BC launches what TD3 launches, with two
small kernels of the actor phase exchanged.  Prints one JSON line and writes it to --out.
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

OBS, ACT, BATCH, HIDDEN = 376, 17, 4096, 256
ALPHA = 2.5


def _stats(times: list[float], steps: int) -> dict:
    med = statistics.median(times)
    return {"updates_per_s_median": steps / med, "updates_per_s_min": steps / max(times), "updates_per_s_max": steps / min(times),
            "us_per_update_median": med / steps * 1e6, "legs": len(times)}


def run(steps: int, warmup: int, legs: int) -> dict:
    import bench_init as BI
    from oracle import oracle_sac as OS
    from tianshou_amd import td3 as T
    from tianshou_amd import td3bc as TB

    if not torch.cuda.is_available():
        raise RuntimeError("bench_td3bc.py measures on an MI355X; there is no CPU path")
    steps, legs = max(2, steps + steps % 2), max(5, legs)            # an even number of updates: every leg steps the actor alike
    actor, c1, c2 = OS.init_td3_params(OBS, ACT, 0, True, HIDDEN)
    flats = (T.actor_flat_from_torch(list(actor.values()), OBS, ACT, hidden=HIDDEN),
             T.critic_flat_from_torch(list(c1.values()), OBS, ACT, hidden=HIDDEN),
             T.critic_flat_from_torch(list(c2.values()), OBS, ACT, hidden=HIDDEN))
    kw = dict(max_action=1.0, actor_lr=3e-4, critic_lr=3e-4, tau=0.005, update_actor_freq=2)
    bc = TB.TD3BCEngine(OBS, ACT, *flats, TB.TD3BCConfig(alpha=ALPHA, **kw), hidden=HIDDEN)
    td3 = T.TD3Engine(OBS, ACT, *flats, T.TD3Config(**kw), hidden=HIDDEN)
    g = torch.Generator(device="cuda").manual_seed(1)
    batches = [(torch.randn(BATCH, OBS, generator=g, device="cuda"), torch.rand(BATCH, ACT, generator=g, device="cuda") * 2 - 1,
                torch.randn(BATCH, generator=g, device="cuda")) for _ in range(8)]

    def leg(eng, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            stats, _ = eng.update_with_batch(*batches[i % len(batches)])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats

    BI.warm_clocks()
    for eng in (bc, td3):
        leg(eng, max(2, warmup + warmup % 2))
    t_bc, t_td3 = [], []
    for i in range(legs):
        order = ((bc, t_bc), (td3, t_td3))
        for eng, sink in (order if i % 2 == 0 else order[::-1]):             # alternate who goes first
            dt, stats = leg(eng, steps)
            sink.append(dt)
            if eng is bc:
                last = stats
    sb, st = _stats(t_bc, steps), _stats(t_td3, steps)
    return {
        "metric": "TD3+BC engine-level updates/sec (obs 376, act 17, B=4096, Net[256, 256], actor every 2nd update)",
        "value": sb["updates_per_s_median"], "unit": "updates/s", **sb, "updates_per_leg": steps, "warmup": warmup,
        "n_gpus": 1, "dtype": "f32", "data": "synthetic", "higher_is_better": True,
        "config": {"workload": f"C5-shape TD3+BC: obs {OBS}, act {ACT}, B={BATCH}, Net[{HIDDEN}, {HIDDEN}], alpha {ALPHA}, "
                               f"update_actor_freq 2, returns supplied"},
        "td3_same_inputs": st, "td3bc_over_td3": sb["updates_per_s_median"] / st["updates_per_s_median"],
        "td3_leg_spread": (max(t_td3) - min(t_td3)) / statistics.median(t_td3),
        "final_stats": [float(x) for x in last.tolist()],
    }


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "td3bc_bench.json"))
    a = ap.parse_args()
    line = json.dumps(run(a.steps, a.warmup, a.legs))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
