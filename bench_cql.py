"""DiscreteCQL on the C3 shape (record, not a gate): B = 512, 84x84x4 uint8 frames, 6 actions, 200 quantiles, n-step 3, lagged
net, PER indices supplied by the device sum-tree -- beside QRDQN on the same inputs in the same process.

    python bench_cql.py [--steps K] [--warmup W] [--slots S] [--out profiles/cql_bench.json]

One "step" = one DiscreteCQL.update(): PER sample -> frame-stack gather of s and s_{t+n} -> both networks on s_{t+n} -> n-step
return of the quantile rows -> forward, quantile Huber + CQL loss, backward, Adam on s -> PER priority update.  The two engines
(DiscreteCQLEngine, DistQEngine kind "qr") start from the same parameters and replay the same index draws on twin sum-trees;
their updates are timed in alternation, each on its own with a device synchronisation, so that clock drift hits both alike.
The expectation is a ratio of 1: the two differ inside one per-sample launch and one scalar reduction.  Also timed: the same
network work in eager PyTorch on the same GPU (tests/oracle_dcql.py moved to the device: two no-grad passes on s_{t+n},
forward + backward + Adam on s; sampling / gather / n-step excluded), and the two head-loss kernels' update calls alone
(gradient-only mode, HIP events).  Prints one JSON line and writes it to --out.
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

C, H, W, N_ACT, BATCH, N = 4, 84, 84, 6, 512, 200
MIN_Q_WEIGHT = 10.0


def eager_baseline(reps: int) -> dict:
    from oracle import oracle_distq as OQ
    from oracle import oracle_dqn as OD
    from tests import oracle_dcql as OC

    cfg = OC.DiscreteCQLConfig(n_atoms=N, gamma=0.99, n_step=3, target_update_freq=500, lr=5e-5, min_q_weight=MIN_Q_WEIGHT)
    p = {k: v.cuda() for k, v in OQ.init_params(C, H, W, N_ACT, N, 0).items()}
    st = OD.DQNState.create(p, cfg.dqn())
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randint(0, 256, (BATCH, C, H, W), generator=g, device="cuda", dtype=torch.uint8)
    obs_next = torch.randint(0, 256, (BATCH, C, H, W), generator=g, device="cuda", dtype=torch.uint8)
    act = torch.randint(0, N_ACT, (BATCH,), generator=g, device="cuda")
    ret = torch.randn((BATCH, N), generator=g, device="cuda")
    w = torch.rand(BATCH, generator=g, device="cuda")

    def one():
        OQ.next_dist(st, cfg, obs_next, N_ACT)
        OC.update_with_batch(st, cfg, obs, act, ret, N_ACT, weight=w)

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
            "what": "tests/oracle_dcql.py on the same GPU (torch eager fp32): 2 no-grad passes on s_{t+n} + fwd/bwd/Adam on s; "
                    "no sampling, gather or n-step arithmetic; the three loss.item() calls synchronise once per update"}


def _event_times(fn, reps: int = 30, warm: int = 5) -> list[float]:
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


def _stats(times: list[float]) -> dict:
    med = statistics.median(times)
    q = statistics.quantiles(times, n=4)
    return {"updates_per_s_median": 1.0 / med, "updates_per_s_min": 1.0 / max(times), "updates_per_s_max": 1.0 / min(times),
            "ms_per_update_median": med * 1e3, "ms_per_update_q1": q[0] * 1e3, "ms_per_update_q3": q[2] * 1e3}


def run(steps: int, warmup: int, slots: int) -> dict:
    import bench_dqn as BD
    import bench_init as BI
    from oracle import oracle_distq as OQ
    from oracle import oracle_dqn as OD
    from tianshou_amd import dcql as CQ
    from tianshou_amd import distq as Q
    from tianshou_amd import dqn as D

    frames, act, buf, per_c = BD.build(slots, 16)
    from tianshou_amd.segtree import PrioritizedWeights

    per_q = PrioritizedWeights(slots, 0.6, 0.4)             # a twin sum-tree for the QRDQN engine, initialised alike
    per_q.init_weight(torch.arange(slots, device="cuda"))
    p = OQ.init_params(C, H, W, N_ACT, N, 0)
    flat = Q.flat_from_torch([p[k] for k in OD.PARAM_ORDER], C, H, W, N_ACT, N)
    kw = dict(n_atoms=N, gamma=0.99, n_step=3, target_update_freq=500, lr=5e-5)
    cql = CQ.DiscreteCQLEngine(C, H, W, N_ACT, flat, CQ.DiscreteCQLConfig(min_q_weight=MIN_Q_WEIGHT, **kw))
    qr = Q.DistQEngine(C, H, W, N_ACT, flat, Q.DistQConfig(kind="qr", **kw))
    gen = torch.Generator(device="cuda").manual_seed(1)

    def update(eng, per, draws):
        idx, wt = per.sample(draws)
        pair = D.gather_obs_pair(frames, buf, idx, 3, C)
        ret = eng.returns_from_obs_next(buf, idx, pair[1])
        loss, td = eng.update_with_batch(pair[0], act[idx], ret, wt)
        per.update_weight(idx, td)
        return loss

    def timed(eng, per, draws):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = update(eng, per, draws)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, loss

    BI.warm_clocks()
    n = max(steps, 20)
    t_c, t_q = [], []
    for i in range(max(warmup, 3) + n):
        draws = torch.rand(BATCH, generator=gen, device="cuda", dtype=torch.float64)
        order = ((cql, per_c, t_c), (qr, per_q, t_q))
        for eng, per, sink in (order if i % 2 == 0 else order[::-1]):      # alternate who goes first
            dt, loss = timed(eng, per, draws)
            if i >= max(warmup, 3):
                sink.append(dt)
            if eng is cql:
                losses = loss
    sc, sq = _stats(t_c), _stats(t_q)

    # the update call alone, gradient-only mode (forward, head loss, reduction, backward; no Adam): where the two engines differ
    idx, wt = per_c.sample(torch.rand(BATCH, generator=gen, device="cuda", dtype=torch.float64))
    pair = D.gather_obs_pair(frames, buf, idx, 3, C)
    ret = cql.returns_from_obs_next(buf, idx, pair[1])
    a = act[idx]
    grad = torch.empty(cql.P, dtype=torch.float32, device="cuda")
    ev_c = _event_times(lambda: cql.update_with_batch(pair[0], a, ret, wt, grad_out=grad, apply=False))
    ev_q = _event_times(lambda: qr.update_with_batch(pair[0], a, ret, wt, grad_out=grad, apply=False))
    eager = eager_baseline(n)
    ratio = sc["ms_per_update_median"] / sq["ms_per_update_median"]
    return {
        "metric": "DiscreteCQL learn() updates/sec (B=512, NatureCNN trunk, 200 quantiles, n-step 3, PER, lagged net)",
        "value": sc["updates_per_s_median"], "unit": "updates/s", **sc, "timed_updates": n, "warmup": max(warmup, 3),
        "n_gpus": 1, "dtype": "f32", "data": "synthetic", "higher_is_better": True,
        "config": {"workload": f"C3-shape DiscreteCQL: {slots} slots of u8[84,84] frames, stack 4, {N_ACT} actions, B={BATCH}, "
                               f"N={N}, n-step 3, PER, target sync every 500, min_q_weight {MIN_Q_WEIGHT}, {cql.P} parameters"},
        "qrdqn_same_inputs": sq, "cql_ms_over_qrdqn_ms": ratio,
        "qrdqn_run_to_run_spread": (sq["ms_per_update_q3"] - sq["ms_per_update_q1"]) / sq["ms_per_update_median"],
        "gradient_only_call_us": {"dcql_median": statistics.median(ev_c), "dcql_min": min(ev_c),
                                  "qrdqn_median": statistics.median(ev_q), "qrdqn_min": min(ev_q),
                                  "note": "HIP events around update_with_batch(apply=False): forward, head loss, reduction, backward"},
        "eager_same_gpu": eager, "engine_vs_eager": sc["updates_per_s_median"] / eager["updates_per_s_median"],
        "final_losses": [float(x) for x in losses.tolist()],
    }


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cql_bench.json"))
    a = ap.parse_args()
    line = json.dumps(run(a.steps, a.warmup, a.slots))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
