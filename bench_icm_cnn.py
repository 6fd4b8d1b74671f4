"""The CNN ICM reward pass and update beside the Atari PPO update they accompany (record, not a gate), engine level.

    python bench_icm_cnn.py [--steps K] [--warmup W] [--legs L] [--out profiles/icm_cnn_bench.json]

Two shapes, both 4 x 84 x 84 uint8 frames, 6 actions, F = 3136, hidden_sizes [512] (examples/atari/atari_ppo.py with
--icm-lr-scale): "atari" -- N = 1,000 transitions per update (10 envs x 100 steps), PPO minibatch 256, repeat 4; "large" --
N = 16,384 (16 envs x 1,024 steps), the same PPO, to show chunking.  Per shape, after a clock warm-up, legs of four kinds alternate
in one process (the order rotates so that clock drift hits all alike); a leg is `--steps` repetitions between two device
synchronisations:
    reward        the rollout's intrinsic reward, chunk by chunk: frame gather (obs and obs_next, uint8 NHWC) + ts_icm_cnn_reward
    update        ICMCnnEngine.update over the same chunks: frame gather + ts_icm_cnn_grad per chunk, ts_icm_cnn_apply (Adam)
    update_eager  the same update in eager PyTorch on the same GPU (tests/oracle_icm_cnn.py on float32 device tensors, whole batch,
                  frames already gathered and converted outside the timed window, statistics kept on the device)
    ppo_update    CnnPPOEngine.update on the same rollout with the augmented rewards (the update ICM accompanies)
"large" adds `update_chunk_<c>` for c in {1024, 4096, 8192}: the same update at that chunk size (`update` uses the default).
The figure of a kind is the median over its legs (`last_stats` of engine and eager agree only at "atari": the chunk legs of "large"
step the engine's model more often than the eager one's).  `conv_gemm_share`: the time of the conv / linear GEMM kernels of ONE update
(conv_fwd + conv_wgrad + conv_dgrad, HIP events around every launch, a run of its own) over the update's time in that same profiled
run -- the rest is the per-row kernels, slab sums, the gather and launch gaps.  Prints one JSON line and writes it to --out.
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

C, H, W, A, HIDDEN = 4, 84, 84, 6, [512]
SHAPES = {"atari": dict(E=10, T=100, batch=256, repeat=4, chunks=()), "large": dict(E=16, T=1024, batch=256, repeat=4, chunks=(1024, 4096, 8192))}
LR, W_FWD, LR_SCALE, REWARD_SCALE = 2.5e-4, 0.2, 1.0, 0.01


def _stats(times: list[float], steps: int) -> dict:
    med = statistics.median(times)
    return {"us_median": med / steps * 1e6, "us_min": min(times) / steps * 1e6, "us_max": max(times) / steps * 1e6, "legs": len(times)}


def algorithmic(n: int) -> dict:
    """What one update needs, from the shapes: multiply-adds x 2 of the three convolutions over 2 N frames and of the two models
    over N rows (forward; the reverse pass costs twice that, conv1 has no input gradient), and the frame bytes read once."""
    f = 3136
    conv = [20 * 20 * 32 * 8 * 8 * C, 9 * 9 * 64 * 4 * 4 * 32, 7 * 7 * 64 * 3 * 3 * 64]
    models = (f + A) * 512 + 512 * f + 2 * f * 512 + 512 * A
    fwd = 2 * (2 * n * sum(conv) + n * models)
    bwd = 2 * (2 * n * (conv[0] + 2 * conv[1] + 2 * conv[2]) + 2 * n * models)
    return {"forward_gflop": fwd / 1e9, "update_gflop": (fwd + bwd) / 1e9, "frame_mbytes": 2 * n * C * H * W / 1e6}


def run_shape(name: str, steps: int, warmup: int, legs: int) -> dict:
    from oracle import oracle_ppo_cnn as OPC
    from tests import oracle_icm_cnn as OC
    from tianshou_amd import icm_cnn as ICC
    from tianshou_amd import ppo_cnn as PC
    from tianshou_amd.buffer import DeviceReplayBuffer, random_permutation
    from tianshou_amd.dqn import gather_obs_nhwc
    from tianshou_amd.icm import ICMConfig
    from tianshou_amd.ppo import PPOConfig

    s = SHAPES[name]
    n = s["E"] * s["T"]
    g = torch.Generator(device="cuda").manual_seed(3)
    frames = torch.randint(0, 256, (n, C, H, W), generator=g, device="cuda", dtype=torch.uint8)
    frames_next = torch.randint(0, 256, (n, C, H, W), generator=g, device="cuda", dtype=torch.uint8)
    act = torch.randint(0, A, (n,), generator=g, device="cuda")
    rew = torch.randn(n, generator=g, device="cuda").double()
    term = torch.rand(n, generator=g, device="cuda") < 0.01
    model = OC.init_model(C, H, W, A, HIDDEN, seed=5)
    # (raw 0..255 frames through fan-in-scaled layers give features of order 10^2 and an mse of order 10^6: conv1 is scaled down so
    # that the update's numbers stay finite over many Adam steps; the arithmetic done per update does not depend on it)
    model[0][0] = model[0][0] / 255.0
    cfg = ICMConfig(lr_scale=LR_SCALE, reward_scale=REWARD_SCALE, forward_loss_weight=W_FWD, lr=LR)
    eng = ICC.ICMCnnEngine(C, H, W, A, HIDDEN, ICC.flat_from_torch(OC.flat_tensors(model), C, H, W, A, HIDDEN, "cuda"), cfg)
    eager = OC.Optim(OC.cast(model, device="cuda"), "adam", lr=LR)
    buf = DeviceReplayBuffer.from_vector_fill(s["E"], obs=frames, act=act, obs_next=frames_next, rew=rew, terminated=term,
                                              truncated=torch.zeros(n, dtype=torch.bool, device="cuda"))
    idx = buf.sample_indices(0)
    act_rows = act[idx]

    def rows(lo, hi):
        i = idx[lo:hi]
        return gather_obs_nhwc(frames, buf, i, 1, as_u8=True), act_rows[lo:hi], gather_obs_nhwc(frames_next, buf, i, 1, as_u8=True)

    def reward(chunk=ICC.DEFAULT_CHUNK):
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        base = rew[idx]
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            out[lo:hi] = eng.reward(*rows(lo, hi), base[lo:hi])
        return out

    p0 = OPC.init_params(C, H, W, A, 1)
    p0["conv1.w"] = p0["conv1.w"] / 255.0
    ppo = PC.CnnPPOEngine(C, H, W, A, PC.flat_from_torch([p0[k] for k in OPC.PARAM_ORDER], C, H, W, A, "cuda"),
                          PPOConfig(lr=LR, max_grad_norm=0.5, vf_coef=0.25, ent_coef=0.01, eps_clip=0.1, value_clip=True))
    pre = ppo.preprocess(buf, frames, act, 1, obs_next_frames=frames_next, chunk=4096, rew=reward())
    perms = [random_permutation(n, 100 + r, "cuda") for r in range(s["repeat"])]
    e_obs, e_act, e_next = rows(0, n)                      # the eager baseline gets its whole batch ready-made

    def op(kind):
        if kind == "reward":
            return reward()
        if kind == "update":
            return eng.update(rows, n=n)
        if kind.startswith("update_chunk_"):
            return eng.update(rows, n=n, chunk=int(kind.rsplit("_", 1)[1]))
        if kind == "update_eager":
            return OC.update(eager, e_obs, e_act, e_next, W_FWD, LR_SCALE)
        return ppo.update(buf, frames, pre, 1, s["batch"], s["repeat"], perms)

    def leg(kind, k):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(k):
            out = op(kind)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    kinds = ["reward", "update", "update_eager", "ppo_update"] + [f"update_chunk_{c}" for c in s["chunks"]]
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
    # one profiled update, a run of its own: HIP events around every conv / linear GEMM launch (side streams folded into one)
    ws = eng._ws
    torch.cuda.synchronize()
    ws.profile_begin()
    t = time.perf_counter()
    eng.update(rows, n=n)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t) * 1e3
    prof = ws.profile_end()
    gemm_ms = sum(prof[k][0] for k in ("conv_fwd", "conv_wgrad", "conv_dgrad"))
    res["profiled_update"] = {"wall_ms": wall_ms, "conv_gemm_ms": gemm_ms, "conv_gemm_launches": sum(prof[k][1] for k in ("conv_fwd", "conv_wgrad", "conv_dgrad")),
                              "by_kind_ms": {k: prof[k][0] for k in ("conv_fwd", "conv_wgrad", "conv_dgrad")}}
    res["conv_gemm_share"] = gemm_ms / wall_ms
    res["config"] = dict(N=n, frame=[C, H, W], A=A, F=eng.feature_dim, hidden_sizes=HIDDEN, chunk=ICC.DEFAULT_CHUNK, ppo_minibatch=s["batch"],
                         ppo_repeat=s["repeat"], ppo_gradient_steps=int(last["ppo_update"][1]), parameters=eng.count)
    res["algorithmic"] = algorithmic(n)
    res["update_tflops"] = res["algorithmic"]["update_gflop"] / res["update"]["us_median"] * 1e3        # (GFLOP per us = 1e3 TFLOP/s)
    res["update_us_per_transition"] = res["update"]["us_median"] / n
    res["eager_over_update"] = res["update_eager"]["us_median"] / res["update"]["us_median"]
    res["icm_over_ppo_update"] = (res["reward"]["us_median"] + res["update"]["us_median"]) / res["ppo_update"]["us_median"]
    res["last_stats"] = {k: [float(x) for x in last[k].tolist()] for k in ("update", "update_eager")}
    if s["chunks"]:
        res["us_per_transition_by_chunk"] = {str(c): res[f"update_chunk_{c}"]["us_median"] / n for c in s["chunks"]}
    return res


def run(steps: int, warmup: int, legs: int) -> dict:
    import bench_init as BI

    if not torch.cuda.is_available():
        raise RuntimeError("bench_icm_cnn.py measures on an MI355X; there is no CPU path")
    legs = max(5, legs)
    BI.warm_clocks()
    small = run_shape("atari", steps, warmup, legs)
    BI.warm_clocks()
    large = run_shape("large", max(1, steps // 10), max(1, warmup // 10), legs)
    return {"metric": "CNN ICM update (frame gather, forward, loss, reverse pass, Adam), engine level (4x84x84 uint8, A 6, F 3136, hidden_sizes [512], N=1000)",
            "value": small["update"]["us_median"], "unit": "us/update", "higher_is_better": False, "n_gpus": 1, "dtype": "f32",
            "data": "synthetic", "steps_per_leg": {"atari": steps, "large": max(1, steps // 10)}, "warmup": warmup,
            "atari": small, "large": large}


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icm_cnn_bench.json"))
    a = ap.parse_args()
    line = json.dumps(run(a.steps, a.warmup, a.legs))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
