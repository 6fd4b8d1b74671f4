"""TEST INFRASTRUCTURE ONLY - generates tests/golden/iqn_lagged.npz and tests/golden/iqn_single.npz by running the
UNMODIFIED reference (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_iqn.py

IQN.update() (tianshou/algorithm/modelfree/iqn.py) on ImplicitQuantileNetwork(DQNet(features_only=True), hidden [512]) over a
synthetic PrioritizedVectorReplayBuffer that stores obs and obs_next.  Per update the file holds the sampled indices, the PER
weights, EVERY fraction tensor the model drew in call order (the model's forward is wrapped: its return value carries them),
the n-step returns [B, N'], the new priorities, the loss, strided parameter samples, all biases and the sum-tree; and once the
buffer contents and the manager state.  The initial parameters are not stored: tests/oracle_iqn.py::init_params rebuilds them
from the seed (checked here against the reference net, tensor by tensor).  Only data is written; nothing of the reference's program text.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

ref_shim.install()

import torch  # noqa: E402
import gymnasium as gym  # noqa: E402  (shim stub)

from tianshou.algorithm.modelfree.iqn import IQN, IQNPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer  # noqa: E402
from tianshou.env.atari.atari_network import DQNet  # noqa: E402
from tianshou.utils.net.discrete import ImplicitQuantileNetwork  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from tests import oracle_iqn as OI  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")

KEYS = ["preprocess.net.0.weight", "preprocess.net.0.bias", "preprocess.net.2.weight", "preprocess.net.2.bias",
        "preprocess.net.4.weight", "preprocess.net.4.bias", "last.model.0.weight", "last.model.0.bias",
        "last.model.2.weight", "last.model.2.bias", "embed_model.net.0.weight", "embed_model.net.0.bias"]


def manager_state(buf) -> dict:
    return {"offset": np.array(buf._extend_offset, np.int64), "last_index": np.array(buf.last_index, np.int64),
            "lengths": np.array(buf._lengths, np.int64),
            "insertion": np.asarray([b._insertion_idx for b in buf.buffers], np.int64)}


def gen_iqn(tag: str, *, E: int, slots: int, steps: int, c: int, h: int, w: int, n_act: int, n_online: int, n_target: int,
            batch: int, n_updates: int, seed: int, lr: float, gamma: float, n_step: int, target_update_freq: int) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    feature_net = DQNet(c=c, h=h, w=w, action_shape=[n_act], features_only=True)
    net = ImplicitQuantileNetwork(preprocess_net=feature_net, action_shape=[n_act], hidden_sizes=[512], num_cosines=64)
    policy = IQNPolicy(model=net, action_space=gym.spaces.Discrete(n_act), sample_size=9, online_sample_size=n_online,
                       target_sample_size=n_target)
    algorithm = IQN(policy=policy, optim=AdamOptimizerFactory(lr=lr), gamma=gamma, n_step_return_horizon=n_step,
                    target_update_freq=target_update_freq)
    assert list(net.state_dict().keys()) == KEYS, list(net.state_dict().keys())

    buf = PrioritizedVectorReplayBuffer(E * slots, E, alpha=0.6, beta=0.4)
    frames = rng.integers(0, 256, size=(steps + 1, E, c, h, w), dtype=np.uint8)
    frames = np.where(rng.random(frames.shape) < 0.06, frames, 0).astype(np.uint8)
    act = rng.integers(0, n_act, size=(steps, E))
    rew = rng.normal(size=(steps, E)).astype(np.float32)
    term = rng.random((steps, E)) < 0.08
    trunc = (rng.random((steps, E)) < 0.04) & ~term
    for t in range(steps):
        buf.add(Batch(obs=frames[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=frames[t + 1]))
    out: dict[str, np.ndarray] = {}
    out["dims"] = np.array([E, slots, steps, c, h, w, n_act, n_online, n_target, batch, n_updates, seed])
    p0 = OI.init_params(c, h, w, n_act, seed=seed)         # the tests rebuild the initial net from the seed
    for k_ref, k in zip(KEYS, OI.PARAM_ORDER):
        assert torch.equal(net.state_dict()[k_ref], p0[k]), f"oracle init differs from the reference net at {k}"
    out["frames"] = np.asarray(buf.obs, np.uint8)
    out["frames_next"] = np.asarray(buf.obs_next, np.uint8)
    out["act"] = np.asarray(buf.act, np.int64)
    out["rew"] = np.asarray(buf.rew, np.float64)
    out["terminated"] = np.asarray(buf.terminated, bool)
    out["truncated"] = np.asarray(buf.truncated, bool)
    for k, v in manager_state(buf).items():
        out["buf_" + k] = v
    out["tree0"] = np.asarray(buf.weight._value, np.float64).copy()

    taus: list[np.ndarray] = []

    def wrap(model):
        orig = model.forward

        def forward(*a, **k):
            r = orig(*a, **k)
            taus.append(r[0][1].detach().numpy().copy())
            return r

        model.forward = forward

    wrap(algorithm.policy.model)
    if algorithm.use_target_network:
        wrap(algorithm.model_old)

    rec: list[dict] = []
    orig_pre, orig_upd = IQN._preprocess_batch, IQN._update_with_batch

    def rec_pre(self, batch, buffer, indices):
        r = {"indices": np.array(indices, np.int64), "is_weight": np.array(batch.weight, np.float64)}
        b = orig_pre(self, batch, buffer, indices)
        r["returns"] = b.returns.numpy().copy()
        rec.append(r)
        return b

    def rec_upd(self, batch):
        stats = orig_upd(self, batch)
        rec[-1]["prio"] = batch.weight.detach().numpy().copy()
        rec[-1]["loss"] = np.array(float(stats.loss))
        return stats

    IQN._preprocess_batch, IQN._update_with_batch = rec_pre, rec_upd
    try:
        np.random.seed(seed + 7)
        for u in range(n_updates):
            taus.clear()
            with policy_within_training_step(algorithm.policy):
                algorithm.update(buffer=buf, sample_size=batch)
            r = rec[-1]
            sd = net.state_dict()
            flat = torch.cat([sd[k].reshape(-1) for k in KEYS]).numpy()
            for k in ("indices", "returns", "prio", "loss", "is_weight"):
                out[f"u{u}_{k}"] = r[k]
            out[f"u{u}_n_taus"] = np.array(len(taus))
            for i, t in enumerate(taus):
                out[f"u{u}_tau{i}"] = t
            out[f"u{u}_params_strided"] = flat[::61].copy()
            out[f"u{u}_conv1_w"] = sd[KEYS[0]].numpy().copy()
            out[f"u{u}_fc2_w"] = sd[KEYS[8]].numpy().copy()
            out[f"u{u}_emb_w_strided"] = sd[KEYS[10]].numpy().reshape(-1)[::7].copy()
            out[f"u{u}_biases"] = torch.cat([sd[k].reshape(-1) for k in KEYS if k.endswith("bias")]).numpy().copy()
            if algorithm.use_target_network:
                old = getattr(algorithm.model_old, "module", algorithm.model_old).state_dict()
                out[f"u{u}_old_params_strided"] = torch.cat([old[k].reshape(-1) for k in KEYS]).numpy()[::61].copy()
            out[f"u{u}_tree"] = np.asarray(buf.weight._value, np.float64).copy()
        opt = algorithm.optim._optim
        params = dict(net.named_parameters())
        st = [opt.state[params[k]] for k in KEYS]
        out["adam_step"] = np.array(int(float(st[0]["step"])))
        out["adam_m_strided"] = torch.cat([s["exp_avg"].reshape(-1) for s in st]).numpy()[::61].copy()
        out["adam_v_strided"] = torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).numpy()[::61].copy()
    finally:
        IQN._preprocess_batch, IQN._update_with_batch = orig_pre, orig_upd
    cfg = dict(gamma=algorithm.gamma, n_step=algorithm.n_step, target_update_freq=algorithm.target_update_freq, lr=lr)
    out["cfg_keys"] = np.array(list(cfg.keys()))
    out["cfg_vals"] = np.array(list(cfg.values()), np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"iqn_{tag}.npz"), **out)


def main() -> None:
    geom = dict(E=3, slots=24, steps=30, c=2, h=44, w=36, batch=24, n_updates=3, lr=3e-4)
    gen_iqn("lagged", n_act=3, n_online=5, n_target=7, seed=17, gamma=0.95, n_step=3, target_update_freq=2, **geom)
    gen_iqn("single", n_act=4, n_online=4, n_target=4, seed=19, gamma=0.9, n_step=1, target_update_freq=0, **geom)


if __name__ == "__main__":
    main()
