"""TEST INFRASTRUCTURE ONLY - generates tests/golden/dcql_lagged.npz and tests/golden/dcql_single.npz by running the
UNMODIFIED reference (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_dcql.py

DiscreteCQL.update() (tianshou/algorithm/imitation/discrete_cql.py) on QRDQNet over a synthetic replay buffer that stores obs
and obs_next: a PrioritizedVectorReplayBuffer with a lagged network and 3-step returns ("lagged"), and the offline case, a
plain VectorReplayBuffer without weights and without a target network ("single").  Per update the file holds the sampled
indices, the PER weights (prioritized buffer only), the n-step returns [B, N], the new priorities, loss / qr_loss / cql_loss,
strided parameter samples, conv1's weights, all biases, the lagged parameters and (prioritized) the sum-tree; once the buffer
contents, the manager state and the Adam moments at the end.  The initial parameters are not stored:
oracle_distq.init_params rebuilds them from the seed (checked here against the reference net, tensor by tensor).  Only data
is written; nothing of the reference's program text.
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

from tianshou.algorithm.imitation.discrete_cql import DiscreteCQL  # noqa: E402
from tianshou.algorithm.modelfree.qrdqn import QRDQNPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.env.atari.atari_network import QRDQNet  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from oracle import oracle_distq as OQ  # noqa: E402
from oracle import oracle_dqn as OD  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
KEYS = OD.TIANSHOU_KEYS


def manager_state(buf) -> dict:
    return {"offset": np.array(buf._extend_offset, np.int64), "last_index": np.array(buf.last_index, np.int64),
            "lengths": np.array(buf._lengths, np.int64),
            "insertion": np.asarray([b._insertion_idx for b in buf.buffers], np.int64)}


def gen_dcql(tag: str, *, prioritized: bool, E: int, slots: int, steps: int, c: int, h: int, w: int, n_act: int, n_atoms: int,
             batch: int, n_updates: int, seed: int, lr: float, gamma: float, n_step: int, target_update_freq: int,
             min_q_weight: float) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    net = QRDQNet(c=c, h=h, w=w, action_shape=[n_act], num_quantiles=n_atoms)
    policy = QRDQNPolicy(model=net, action_space=gym.spaces.Discrete(n_act))
    algorithm = DiscreteCQL(policy=policy, optim=AdamOptimizerFactory(lr=lr), min_q_weight=min_q_weight, gamma=gamma,
                            num_quantiles=n_atoms, n_step_return_horizon=n_step, target_update_freq=target_update_freq)
    assert list(net.state_dict().keys()) == KEYS, list(net.state_dict().keys())
    p0 = OQ.init_params(c, h, w, n_act, n_atoms, seed)          # the tests rebuild the initial net from the seed
    for k_ref, k in zip(KEYS, OD.PARAM_ORDER):
        assert torch.equal(net.state_dict()[k_ref], p0[k]), f"oracle init differs from the reference net at {k}"

    if prioritized:
        buf = PrioritizedVectorReplayBuffer(E * slots, E, alpha=0.6, beta=0.4)
    else:
        buf = VectorReplayBuffer(E * slots, E)
    frames = rng.integers(0, 256, size=(steps + 1, E, c, h, w), dtype=np.uint8)
    frames = np.where(rng.random(frames.shape) < 0.06, frames, 0).astype(np.uint8)
    act = rng.integers(0, n_act, size=(steps, E))
    rew = rng.normal(size=(steps, E)).astype(np.float32)
    term = rng.random((steps, E)) < 0.08
    trunc = (rng.random((steps, E)) < 0.04) & ~term
    for t in range(steps):
        buf.add(Batch(obs=frames[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=frames[t + 1]))
    out: dict[str, np.ndarray] = {}
    out["dims"] = np.array([E, slots, steps, c, h, w, n_act, n_atoms, batch, n_updates, seed, int(prioritized)])
    out["frames"] = np.asarray(buf.obs, np.uint8)
    out["frames_next"] = np.asarray(buf.obs_next, np.uint8)
    out["act"] = np.asarray(buf.act, np.int64)
    out["rew"] = np.asarray(buf.rew, np.float64)
    out["terminated"] = np.asarray(buf.terminated, bool)
    out["truncated"] = np.asarray(buf.truncated, bool)
    for k, v in manager_state(buf).items():
        out["buf_" + k] = v
    if prioritized:
        out["tree0"] = np.asarray(buf.weight._value, np.float64).copy()

    rec: list[dict] = []
    orig_pre, orig_upd = DiscreteCQL._preprocess_batch, DiscreteCQL._update_with_batch

    def rec_pre(self, batch, buffer, indices):
        r = {"indices": np.array(indices, np.int64)}
        if prioritized:
            r["is_weight"] = np.array(batch.weight, np.float64)
        else:
            assert "weight" not in batch.get_keys()
        b = orig_pre(self, batch, buffer, indices)
        r["returns"] = b.returns.numpy().copy()
        rec.append(r)
        return b

    def rec_upd(self, batch):
        stats = orig_upd(self, batch)
        rec[-1]["prio"] = batch.weight.detach().numpy().copy()
        rec[-1]["loss"] = np.array(float(stats.loss))
        rec[-1]["qr_loss"] = np.array(float(stats.qr_loss))
        rec[-1]["cql_loss"] = np.array(float(stats.cql_loss))
        return stats

    DiscreteCQL._preprocess_batch, DiscreteCQL._update_with_batch = rec_pre, rec_upd
    try:
        np.random.seed(seed + 7)
        for u in range(n_updates):
            with policy_within_training_step(algorithm.policy):
                algorithm.update(buffer=buf, sample_size=batch)
            r = rec[-1]
            sd = net.state_dict()
            flat = torch.cat([sd[k].reshape(-1) for k in KEYS]).numpy()
            for k, v in r.items():
                out[f"u{u}_{k}"] = v
            out[f"u{u}_params_strided"] = flat[::61].copy()
            out[f"u{u}_conv1_w"] = sd[KEYS[0]].numpy().copy()
            out[f"u{u}_biases"] = torch.cat([sd[k].reshape(-1) for k in KEYS if k.endswith("bias")]).numpy().copy()
            if algorithm.use_target_network:
                old = getattr(algorithm.model_old, "module", algorithm.model_old).state_dict()
                out[f"u{u}_old_params_strided"] = torch.cat([old[k].reshape(-1) for k in KEYS]).numpy()[::61].copy()
            if prioritized:
                out[f"u{u}_tree"] = np.asarray(buf.weight._value, np.float64).copy()
        opt = algorithm.optim._optim
        params = dict(net.named_parameters())
        st = [opt.state[params[k]] for k in KEYS]
        out["adam_step"] = np.array(int(float(st[0]["step"])))
        out["adam_m_strided"] = torch.cat([s["exp_avg"].reshape(-1) for s in st]).numpy()[::61].copy()
        out["adam_v_strided"] = torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).numpy()[::61].copy()
    finally:
        DiscreteCQL._preprocess_batch, DiscreteCQL._update_with_batch = orig_pre, orig_upd
    cfg = dict(gamma=algorithm.gamma, n_step=algorithm.n_step, target_update_freq=algorithm.target_update_freq, lr=lr,
               min_q_weight=algorithm.min_q_weight)
    out["cfg_keys"] = np.array(list(cfg.keys()))
    out["cfg_vals"] = np.array(list(cfg.values()), np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"dcql_{tag}.npz"), **out)


def main() -> None:
    geom = dict(E=3, slots=24, steps=30, c=2, h=44, w=36, batch=24, n_updates=3, lr=3e-4)
    gen_dcql("lagged", prioritized=True, n_act=3, n_atoms=21, seed=23, gamma=0.95, n_step=3, target_update_freq=2,
             min_q_weight=10.0, **geom)
    gen_dcql("single", prioritized=False, n_act=4, n_atoms=8, seed=29, gamma=0.9, n_step=1, target_update_freq=0,
             min_q_weight=0.5, **geom)


if __name__ == "__main__":
    main()
