"""IQN on the C3 shape (record, not a gate): B = 512, 84x84x4 uint8 frames, 6 actions, N = N' = 8, K = 64 cosines, n-step 3,
lagged net, PER indices supplied by the device sum-tree.

    python bench_iqn.py [--steps K] [--warmup W] [--slots S]

One "step" = one IQN.update(): PER sample -> frame-stack gather of s and s_{t+n} -> both networks on s_{t+n} (fractions from
the engine's own stream) -> n-step return of the quantile rows -> forward, quantile Huber loss, backward, Adam on s -> PER
priority update.  Prints one JSON line: engine updates/s (median and min over the timed updates, each timed on its own with a
device synchronisation), the same network work in eager PyTorch on the same GPU (tests/oracle_iqn.py moved to the device:
two no-grad passes on s_{t+n}, forward + backward + Adam on s; sampling / gather / n-step excluded), and the two cosine-
embedding kernels alone from HIP events with their fraction of the fp32-MFMA peak (forward 2 R K F flop; backward twice that
plus the recomputed forward product).
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

C, H, W, N_ACT, BATCH, N, K, F = 4, 84, 84, 6, 512, 8, 64, 3136
PEAK_F32_MFMA_TFLOPS = 157.3


def _event_times(fn, reps: int = 20, warm: int = 3) -> list[float]:
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def embed_kernels() -> dict:
    from tianshou_amd import iqn as I

    g = torch.Generator(device="cuda").manual_seed(0)
    tau = torch.rand((BATCH, N), generator=g, device="cuda")
    feat = torch.relu(torch.randn((BATCH, F), generator=g, device="cuda"))
    we_be = (torch.randn((K + 1, F), generator=g, device="cuda") * 0.1).contiguous()
    dx = torch.randn((BATCH * N, F), generator=g, device="cuda")
    R = BATCH * N
    x, grads = torch.empty((R, F), device="cuda"), (torch.empty_like(feat), torch.empty_like(we_be))
    flop_f, flop_b = 2 * R * K * F, 3 * 2 * R * K * F
    res = {}
    for route in ("fused", "unfused"):        # the one-launch kernels against the route through the generic GEMM kernels
        fwd = _event_times(lambda: I.embed_mul(tau, feat, we_be, out=x, route=route))
        bwd = _event_times(lambda: I.embed_mul_backward(tau, feat, we_be, dx, out=grads, route=route))
        for name, t, flop, byts in (("iqn_embed_mul_forward", fwd, flop_f, 4 * R * F + 4 * BATCH * F),
                                    ("iqn_embed_mul_backward", bwd, flop_b, 4 * R * F + 8 * BATCH * F)):
            med = statistics.median(t)
            tf = flop / (med * 1e-6) / 1e12
            res[f"{name}_{route}"] = {"us_median": med, "us_min": min(t), "flop": flop, "algorithmic_bytes": byts, "tflops": tf,
                                      "frac_of_f32_mfma_peak": tf / PEAK_F32_MFMA_TFLOPS,
                                      "gbytes_per_s": byts / (med * 1e-6) / 1e9}
    res["note"] = ("HIP events around single calls of ts_iqn_embed_mul / ts_iqn_embed_mul_backward (preallocated outputs; the backward call includes "
                   "its slab sum), R = 4096 rows, F = 3136, K = 64; flop / bytes are the algorithmic ones of the fused form for both routes")
    return res


def eager_baseline(reps: int) -> dict:
    from oracle import oracle_dqn as OD
    from tests import oracle_iqn as OI

    cfg = OI.IQNConfig(gamma=0.99, n_step=3, target_update_freq=500, lr=1e-4)
    p = {k: v.cuda() for k, v in OI.init_params(C, H, W, N_ACT, seed=0).items()}
    st = OD.DQNState.create(p, cfg.dqn())
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randint(0, 256, (BATCH, C, H, W), generator=g, device="cuda", dtype=torch.uint8)
    obs_next = torch.randint(0, 256, (BATCH, C, H, W), generator=g, device="cuda", dtype=torch.uint8)
    act = torch.randint(0, N_ACT, (BATCH,), generator=g, device="cuda")
    ret = torch.randn((BATCH, N), generator=g, device="cuda")
    w = torch.rand(BATCH, generator=g, device="cuda")

    def one():
        OI.next_dist(st, obs_next, torch.rand((BATCH, N), device="cuda"), torch.rand((BATCH, N), device="cuda"))
        OI.update_with_batch(st, cfg, obs, act, ret, torch.rand((BATCH, N), device="cuda"), weight=w)

    times = []
    for i in range(3 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    return {"updates_per_s_median": 1.0 / med, "updates_per_s_min": 1.0 / max(times), "ms_median": med * 1e3, "updates": reps,
            "what": "tests/oracle_iqn.py on the same GPU (torch eager fp32): 2 no-grad passes on s_{t+n} + fwd/bwd/Adam on s; "
                    "no sampling, gather or n-step arithmetic; loss.item() synchronises once per update"}


def run(steps: int, warmup: int, slots: int) -> dict:
    import bench_dqn as BD
    import bench_init as BI
    from tianshou_amd import dqn as D
    from tianshou_amd import iqn as I
    from tests import oracle_iqn as OI

    frames, act, buf, per = BD.build(slots, 16)
    p = OI.init_params(C, H, W, N_ACT, seed=0)
    cfg = I.IQNConfig(sample_size=32, online_sample_size=N, target_sample_size=N, gamma=0.99, n_step=3, target_update_freq=500,
                      lr=1e-4, seed=1)
    eng = I.IQNEngine(C, H, W, N_ACT, I.flat_from_torch([p[k] for k in OI.PARAM_ORDER], C, H, W, N_ACT), cfg)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def update():
        idx, wt = per.sample(torch.rand(BATCH, generator=gen, device="cuda", dtype=torch.float64))
        pair = D.gather_obs_pair(frames, buf, idx, cfg.n_step, C)
        ret = eng.returns_from_obs_next(buf, idx, pair[1])
        loss, td = eng.update_with_batch(pair[0], act[idx], ret, wt)
        per.update_weight(idx, td)
        return loss

    BI.warm_clocks()
    for _ in range(max(warmup, 3)):
        update()
    times = []
    for _ in range(max(steps, 20)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = update()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(max(steps, 20)):
        loss = update()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / max(steps, 20)
    med = statistics.median(times)
    eager = eager_baseline(max(steps, 20))
    return {
        "metric": "IQN learn() updates/sec (B=512, NatureCNN trunk, N=N'=8, 64 cosines, n-step 3, PER, lagged net)",
        "value": 1.0 / med, "unit": "updates/s", "updates_per_s_median": 1.0 / med, "updates_per_s_min": 1.0 / max(times),
        "updates_per_s_back_to_back": 1.0 / dt, "ms_per_update_median": med * 1e3, "timed_updates": len(times), "warmup": max(warmup, 3),
        "n_gpus": 1, "dtype": "f32", "data": "synthetic", "higher_is_better": True,
        "config": {"workload": f"C3-shape IQN: {slots} slots of u8[84,84] frames, stack 4, {N_ACT} actions, B={BATCH}, "
                               f"N=N'={N}, K={K}, n-step 3, PER, target sync every 500, {eng.P} parameters"},
        "eager_same_gpu": eager, "engine_vs_eager": (1.0 / med) / eager["updates_per_s_median"],
        "embed_kernels": embed_kernels(), "final_loss": float(loss),
    }


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 18)
    a = ap.parse_args()
    print(json.dumps(run(a.steps, a.warmup, a.slots)), flush=True)
