"""TEST INFRASTRUCTURE ONLY - the inputs of tests/test_gpu_icm_cnn_edges.py, built on the CPU from frozen `np.random.RandomState`
streams so that the float32-vs-float64 distance of the oracle on the very same inputs can be measured without a GPU
(`python -m tests.icm_cnn_cases` prints it per case; the bars of the GPU tests that are not the project's default quote it)."""
from __future__ import annotations

import os

import numpy as np
import torch

from tests import oracle_icm_cnn as OC

W_FWD, LR_SCALE, LR = 0.2, 1.0, 1e-3

# (h, w, B, A, model_hidden): every frame size of the issue, B in {1, 63, 64, 65} (64 rows per loss workgroup), A in {1, 18, 33, 64},
# hidden (), [48, 80], [512]; 84 x 84 at B = 5 is the only F = 3136 case
SHAPES = {
    "36x36": (36, 36, 5, 6, [64]),
    "44x36_b1_a1": (44, 36, 1, 1, []),
    "44x44_b63_a18": (44, 44, 63, 18, [48, 80]),
    "36x36_b64_a33": (36, 36, 64, 33, [512]),
    "36x36_b65_a64": (36, 36, 65, 64, []),
    "84x84": (84, 84, 5, 6, [512]),
}
_CACHE: dict = {}


def frames(rs: np.random.RandomState, b: int, h: int, w: int, c: int = 4) -> torch.Tensor:
    return torch.from_numpy(rs.randint(0, 256, size=(b, h, w, c)).astype(np.uint8))


def case(name: str, c: int = 4) -> dict:
    """-> {model (float32 tensor lists), obs, act, obs_next (uint8 NHWC / int64), rew, dims} of SHAPES[name]."""
    if name not in _CACHE:
        h, w, b, a, mh = SHAPES[name]
        seed = 1000 + sorted(SHAPES).index(name)
        rs = np.random.RandomState(seed)
        _CACHE[name] = dict(model=OC.init_model(c, h, w, a, mh, seed), obs=frames(rs, b, h, w, c), obs_next=frames(rs, b, h, w, c),
                            act=torch.from_numpy(rs.randint(0, a, size=b).astype(np.int64)), rew=torch.from_numpy(rs.normal(size=b)),
                            dims=(c, h, w, a, mh))
    return _CACHE[name]


def reference(name: str, dtype=torch.float64, device="cpu") -> dict:
    """The oracle on case(name): mse, act_hat, stats, grads at the initial model and the model after one Adam step (computed once)."""
    key = (name, dtype, str(device))
    if key not in _CACHE:
        cs = case(name)
        model = OC.cast(cs["model"], dtype, device)
        obs, act, nxt = cs["obs"].to(device), cs["act"].to(device), cs["obs_next"].to(device)
        stats, gs, mse, act_hat = OC.grads(model, obs, act, nxt, W_FWD, LR_SCALE)
        opt = OC.Optim(model, "adam", lr=LR)
        OC.update(opt, obs, act, nxt, W_FWD, LR_SCALE)
        _CACHE[key] = dict(stats=stats, grads=gs, mse=mse, act_hat=act_hat, after=opt.model())
    return _CACHE[key]


def cat(model) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1).double().cpu() for chain in model for t in chain]).numpy()


def distances(name: str) -> dict:
    """float32 oracle vs float64 oracle on the CPU: the largest relative error of mse / statistics / act_hat (relative to the
    largest |act_hat|), the gradient's largest error over its largest entry, the post-step parameters' largest error over lr."""
    a, b = reference(name, torch.float32), reference(name, torch.float64)
    rel = lambda x, y: float(((x.double() - y).abs() / y.abs()).max())  # noqa: E731
    ga, gb = cat(a["grads"]), cat(b["grads"])
    return dict(mse=rel(a["mse"], b["mse"]), stats=rel(a["stats"], b["stats"]),
                act_hat=float((a["act_hat"].double() - b["act_hat"]).abs().max() / b["act_hat"].abs().max()),
                grad=float(np.abs(ga - gb).max() / np.abs(gb).max()), params_over_lr=float(np.abs(cat(a["after"]) - cat(b["after"])).max() / LR))


if __name__ == "__main__":
    for n in SHAPES:
        print(n, {k: f"{v:.2e}" for k, v in distances(n).items()})


# ---- the reference's recorded runs (tests/golden/icm_cnn_*.npz, tools/gen_golden_icm_cnn.py) ---------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(tag: str) -> dict:
    key = ("golden", tag)
    if key not in _CACHE:
        g = dict(np.load(os.path.join(GOLDEN, f"icm_cnn_{tag}.npz")))
        g["cfg"] = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
        E, T, c, h, w, a, bsz, rep, seed, n_upd, stride, stacked, f_dim = (int(x) for x in g["dims"])
        g["d"] = dict(E=E, T=T, c=c, h=h, w=w, n_act=a, batch_size=bsz, repeat=rep, seed=seed, stride=stride, stacked=bool(stacked),
                      f_dim=f_dim, model_hidden=g["model_hidden"].tolist())
        _CACHE[key] = g
    return _CACHE[key]


def fixture_model(g, dtype=torch.float32):
    """The ICM model's initial parameters, rebuilt from the stored seed."""
    d = g["d"]
    return OC.init_model(d["c"], d["h"], d["w"], d["n_act"], d["model_hidden"], d["seed"] + 1, dtype)


def fixture_ppo(g) -> list[torch.Tensor]:
    d = g["d"]
    return OC.init_ppo(d["c"], d["h"], d["w"], d["n_act"], d["seed"])


def fixture_rows(g, u: int = 0):
    """-> (obs, act, obs_next, rew_before) of update u: uint8 NHWC frames as buffer[indices] yields them (stacked where the
    buffer stacks; obs_next = the stored column or, without one, the observation at next(index))."""
    from oracle import oracle as O
    from oracle import oracle_dqn as OD

    d, idx = g["d"], g[f"u{u}_pre_indices"]
    if d["stacked"]:
        bs = O.BufferState.from_vector_fill(g["rew"], g["terminated"], g["truncated"], d["E"])
        obs = OD.stacked_frames(bs, g["obs"], idx, d["c"])
        nxt = OD.stacked_frames(bs, g["obs"], g[f"u{u}_pre_next_indices"], d["c"])
    else:
        obs, nxt = g["obs"][idx], g["obs_next"][idx]
    nhwc = lambda x: torch.from_numpy(np.ascontiguousarray(x)).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    return nhwc(obs), torch.from_numpy(g["act"][idx]), nhwc(nxt), torch.from_numpy(g[f"u{u}_pre_rew_before"])
