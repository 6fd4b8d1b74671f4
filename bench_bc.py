"""Behaviour cloning (record, not a gate): engine-level updates beside the parent engine's update and eager PyTorch on the same
inputs in the same process.

    python bench_bc.py [--steps K] [--warmup W] [--legs L] [--shapes atari32,atari512,d4rl,c5] [--out profiles/bc_bench.json]

Shapes: examples/offline/atari_il.py's (DQNet 4x84x84, 6 actions, u8 frames) at B = 32 and B = 512; examples/offline/d4rl_il.py's
(obs 17, act 6, Net[256, 256], B = 256); the C5 shape (obs 376, act 17, Net[256, 256], B = 4096).  One "update" = one
`update_with_batch` on a batch already on the device.  Three legs per shape:
    bc       tianshou_amd.bc (BCDQNetEngine / BCMlpEngine continuous)
    parent   the engine whose trunk it shares, with returns supplied: DQNEngine.update_with_batch (no target network), or
             TD3Engine.update_with_batch (two critic steps, the actor step on every second update)
    eager    the same update in eager PyTorch on the same GPU (tests/oracle_bc.py on device tensors; `loss.item()` per update,
             as the reference's `_imitation_update`)
A leg is `--steps` updates between two device synchronisations; the legs alternate after a clock warm-up, so that clock drift
hits all alike, and every figure is the median over at least 7 legs each.  The update does less network work than its parent's
on the same rows, so `bc_over_parent_time` (median time per update, bc / parent) is expected below 1.  Prints one JSON line and
writes it to --out.
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

SHAPES = {"atari32": ("dqnet", 32), "atari512": ("dqnet", 512), "d4rl": ("mlp", 256, 17, 6), "c5": ("mlp", 4096, 376, 17)}
C, H, W, N_ACT, HIDDEN = 4, 84, 84, 6, 256


def _stats(times: list[float], steps: int) -> dict:
    med = statistics.median(times)
    return {"updates_per_s_median": steps / med, "us_per_update_median": med / steps * 1e6,
            "us_per_update_min": min(times) / steps * 1e6, "us_per_update_max": max(times) / steps * 1e6, "legs": len(times)}


def _legs(engines: dict, steps: int, warmup: int, legs: int) -> dict:
    """engines: name -> (step function i -> None, updates per leg).  Alternating legs, rotating who goes first."""
    import bench_init as BI

    def leg(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            fn(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    BI.warm_clocks()
    names = list(engines)
    for k in names:
        leg(engines[k][0], max(2, min(warmup, engines[k][1])))
    times = {k: [] for k in names}
    for i in range(legs):
        for k in names[i % len(names):] + names[:i % len(names)]:
            times[k].append(leg(*engines[k]))
    return {k: _stats(times[k], engines[k][1]) for k in names}


def run_dqnet(batch: int, steps: int, warmup: int, legs: int) -> dict:
    from oracle import oracle_dqn as OD
    from tests import oracle_bc as OB
    from tianshou_amd import bc as BC
    from tianshou_amd import dqn as D

    p = OD.init_params(C, H, W, N_ACT, 0)
    flat = D.flat_from_torch([p[k] for k in OD.PARAM_ORDER], C, H, W, N_ACT)
    bc = BC.BCDQNetEngine(C, H, W, N_ACT, flat, BC.BCConfig(lr=1e-4))
    dqn = D.DQNEngine(C, H, W, N_ACT, flat, D.DQNConfig(lr=1e-4, target_update_freq=0))
    ocfg = OD.DQNConfig(lr=1e-4)
    st = OD.DQNState.create({k: v.cuda() for k, v in p.items()}, ocfg)
    g = torch.Generator(device="cuda").manual_seed(1)
    batches = []
    for _ in range(4):
        obs = torch.randint(0, 256, (batch, H, W, C), generator=g, device="cuda", dtype=torch.uint8)
        batches.append((obs, obs.permute(0, 3, 1, 2).contiguous(), torch.randint(0, N_ACT, (batch,), generator=g, device="cuda"),
                        torch.randn(batch, generator=g, device="cuda")))
    n = len(batches)
    eager_steps = max(2, steps // 4)
    out = _legs({"bc": (lambda i: bc.update_with_batch(batches[i % n][0], batches[i % n][2]), steps),
                 "parent": (lambda i: dqn.update_with_batch(batches[i % n][0], batches[i % n][2], batches[i % n][3]), steps),
                 "eager": (lambda i: OB.update_with_batch(st, ocfg, "dqnet", batches[i % n][1], batches[i % n][2]), eager_steps)},
                steps, warmup, legs)
    out["parent_engine"] = "DQNEngine.update_with_batch (returns supplied, no target network)"
    out["workload"] = f"DQNet {C}x{H}x{W}, {N_ACT} actions, u8 frames, B={batch}"
    return out


def run_mlp(batch: int, obs_dim: int, act_dim: int, steps: int, warmup: int, legs: int) -> dict:
    from oracle import oracle_dqn as OD
    from oracle import oracle_sac as OS
    from tests import oracle_bc as OB
    from tianshou_amd import bc as BC
    from tianshou_amd import td3 as T

    steps += steps % 2                                              # an even number of updates: every TD3 leg steps the actor alike
    actor, c1, c2 = OS.init_td3_params(obs_dim, act_dim, 0, True, HIDDEN)
    fa = T.actor_flat_from_torch(list(actor.values()), obs_dim, act_dim, hidden=HIDDEN)
    bc = BC.BCMlpEngine("continuous", obs_dim, act_dim, fa, BC.BCConfig(lr=3e-4, max_action=1.0), hidden=HIDDEN)
    td3 = T.TD3Engine(obs_dim, act_dim, fa, T.critic_flat_from_torch(list(c1.values()), obs_dim, act_dim, hidden=HIDDEN),
                      T.critic_flat_from_torch(list(c2.values()), obs_dim, act_dim, hidden=HIDDEN),
                      T.TD3Config(max_action=1.0, actor_lr=3e-4, critic_lr=3e-4, tau=0.005, update_actor_freq=2), hidden=HIDDEN)
    ocfg = OD.DQNConfig(lr=3e-4)
    st = OD.DQNState.create({k: v.cuda() for k, v in actor.items()}, ocfg)
    g = torch.Generator(device="cuda").manual_seed(1)
    batches = [(torch.randn(batch, obs_dim, generator=g, device="cuda"), torch.rand(batch, act_dim, generator=g, device="cuda") * 2 - 1,
                torch.randn(batch, generator=g, device="cuda")) for _ in range(8)]
    n = len(batches)
    out = _legs({"bc": (lambda i: bc.update_with_batch(*batches[i % n][:2]), steps),
                 "parent": (lambda i: td3.update_with_batch(*batches[i % n]), steps),
                 "eager": (lambda i: OB.update_with_batch(st, ocfg, "continuous", *batches[i % n][:2]), steps)},
                steps, warmup, legs)
    out["parent_engine"] = "TD3Engine.update_with_batch (returns supplied, two critics, actor on every second update)"
    out["workload"] = f"ContinuousActorDeterministic over Net[{HIDDEN}, {HIDDEN}], obs {obs_dim}, act {act_dim}, B={batch}"
    return out


def run(steps: int, warmup: int, legs: int, shapes: list[str]) -> dict:
    if not torch.cuda.is_available():
        raise RuntimeError("bench_bc.py measures on an MI355X; there is no CPU path")
    legs = max(7, legs)
    res = {}
    for name in shapes:
        spec = SHAPES[name]
        r = run_dqnet(spec[1], steps, warmup, legs) if spec[0] == "dqnet" else run_mlp(*spec[1:], steps, warmup, legs)
        r["bc_over_parent_time"] = r["bc"]["us_per_update_median"] / r["parent"]["us_per_update_median"]
        r["eager_over_bc_time"] = r["eager"]["us_per_update_median"] / r["bc"]["us_per_update_median"]
        res[name] = r
    first = res[shapes[0]]
    return {"metric": f"behaviour-cloning engine-level updates/sec ({first['workload']})", "value": first["bc"]["updates_per_s_median"],
            "unit": "updates/s", "updates_per_leg": steps, "warmup": warmup, "n_gpus": 1, "dtype": "f32", "data": "synthetic",
            "higher_is_better": True, "shapes": res}


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc_bench.json"))
    a = ap.parse_args()
    line = json.dumps(run(a.steps, a.warmup, a.legs, [s for s in a.shapes.split(",") if s]))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
