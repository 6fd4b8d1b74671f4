"""TEST INFRASTRUCTURE ONLY - generates tests/golden/bcq_masked.npz and tests/golden/bcq_plain.npz by running the
UNMODIFIED reference (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_bcq.py

DiscreteBCQ.update() (tianshou/algorithm/imitation/discrete_bcq.py) on two DiscreteActor heads over one
DQNet(features_only=True) trunk, as examples/offline/atari_bcq.py builds them, over a synthetic plain VectorReplayBuffer that
stores obs and obs_next: a threshold that really masks actions with 3-step returns ("masked"), and a threshold of 0 with a
strong logit penalty and 1-step returns ("plain").  Per update the file holds the sampled indices, the n-step returns, the
action of the target pass, loss / q_loss / i_loss / reg_loss, strided parameter samples, all biases and the lagged strided
parameters; once the buffer contents, the manager state and the Adam moments at the end.  The initial parameters are not
stored: tests/oracle_bcq.init_params rebuilds them from the seed (checked here against the reference net, tensor by tensor).
Only data is written; nothing of the reference's program text.

Three conditions are asserted, so that a fixture cannot pass vacuously or sit on a knife edge:
  1. "masked": the masked argmax differs from the plain argmax in at least 25 % of the rows of every policy pass;
  2. every |ratio - float32(log tau)| is >= 1e-3;
  3. the gap between the two largest allowed Q values is >= 1e-3 in every row of every policy pass.
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

from tianshou.algorithm.imitation.discrete_bcq import DiscreteBCQ, DiscreteBCQPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou.env.atari.atari_network import DQNet  # noqa: E402
from tianshou.utils.net.discrete import DiscreteActor  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from tests import oracle_bcq as OB  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
KEYS = OB.TIANSHOU_KEYS
OLD_KEYS = [k[len("model."):] for k in KEYS[:10]]
STRIDE = 61


def manager_state(buf) -> dict:
    return {"offset": np.array(buf._extend_offset, np.int64), "last_index": np.array(buf.last_index, np.int64),
            "lengths": np.array(buf._lengths, np.int64),
            "insertion": np.asarray([b._insertion_idx for b in buf.buffers], np.int64)}


def gen_bcq(tag: str, *, E: int, slots: int, steps: int, c: int, h: int, w: int, n_act: int, batch: int, n_updates: int, seed: int,
            lr: float, gamma: float, n_step: int, target_update_freq: int, threshold: float, penalty: float) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    feature_net = DQNet(c=c, h=h, w=w, action_shape=n_act, features_only=True)
    model = DiscreteActor(preprocess_net=feature_net, action_shape=n_act, hidden_sizes=[512], softmax_output=False)
    imitator = DiscreteActor(preprocess_net=feature_net, action_shape=n_act, hidden_sizes=[512], softmax_output=False)
    policy = DiscreteBCQPolicy(model=model, imitator=imitator, action_space=gym.spaces.Discrete(n_act),
                               unlikely_action_threshold=threshold, target_update_freq=target_update_freq)
    algorithm = DiscreteBCQ(policy=policy, optim=AdamOptimizerFactory(lr=lr), gamma=gamma, n_step_return_horizon=n_step,
                            target_update_freq=target_update_freq, imitation_logits_penalty=penalty)
    named = dict(policy.named_parameters())
    assert list(named.keys()) == KEYS, list(named.keys())
    assert model.preprocess is imitator.preprocess
    assert len(algorithm.optim._optim.param_groups) == 1 and len(algorithm.optim._optim.param_groups[0]["params"]) == 14
    old_mod = getattr(algorithm.model_old, "module", algorithm.model_old)
    assert list(dict(old_mod.named_parameters()).keys()) == OLD_KEYS
    p0 = OB.init_params(c, h, w, n_act, seed)                    # the tests rebuild the initial net from the seed
    for k_ref, k in zip(KEYS, OB.PARAM_ORDER):
        assert torch.equal(named[k_ref], p0[k]), f"oracle init differs from the reference net at {k}"

    # the buffer draws its indices from a generator of its own: seeded here, so that the file does not depend on its default.
    # seed + 1 is the first offset at which both files meet the three conditions below (0 and 7 miss the threshold distance)
    buf = VectorReplayBuffer(E * slots, E, random_seed=seed + 1)
    frames = rng.integers(0, 256, size=(steps + 1, E, c, h, w), dtype=np.uint8)
    frames = np.where(rng.random(frames.shape) < 0.06, frames, 0).astype(np.uint8)
    act = rng.integers(0, n_act, size=(steps, E))
    rew = rng.normal(size=(steps, E)).astype(np.float32)
    term = rng.random((steps, E)) < 0.08
    trunc = (rng.random((steps, E)) < 0.04) & ~term
    for t in range(steps):
        buf.add(Batch(obs=frames[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=frames[t + 1]))
    out: dict[str, np.ndarray] = {}
    out["dims"] = np.array([E, slots, steps, c, h, w, n_act, batch, n_updates, seed])
    out["frames"] = np.asarray(buf.obs, np.uint8)
    out["frames_next"] = np.asarray(buf.obs_next, np.uint8)
    out["act"] = np.asarray(buf.act, np.int64)
    out["rew"] = np.asarray(buf.rew, np.float64)
    out["terminated"] = np.asarray(buf.terminated, bool)
    out["truncated"] = np.asarray(buf.truncated, bool)
    for k, v in manager_state(buf).items():
        out["buf_" + k] = v

    rec: list[dict] = []
    passes: list[dict] = []
    log_tau32 = np.float32(policy._log_tau)
    orig_fwd, orig_pre, orig_upd = DiscreteBCQPolicy.forward, DiscreteBCQ._preprocess_batch, DiscreteBCQ._update_with_batch

    def rec_fwd(self, batch, state=None, model=None):
        res = orig_fwd(self, batch, state=state, model=model)
        q = res.q_value.detach().numpy().astype(np.float32)
        lg = res.imitation_logits.detach().numpy().astype(np.float32)
        ratio = lg - lg.max(axis=1, keepdims=True)
        allowed = ~(ratio < log_tau32)
        qa = np.where(allowed, q, -np.inf)
        top2 = np.sort(qa, axis=1)[:, ::-1][:, :2] if n_act > 1 else np.concatenate([qa, np.full_like(qa, -np.inf)], 1)
        passes.append({"act": np.asarray(res.act.detach().numpy(), np.int64), "changed": float((qa.argmax(1) != q.argmax(1)).mean()),
                       "dist": float(np.abs(ratio.astype(np.float64) - float(log_tau32)).min()),
                       "gap": float((top2[:, 0] - top2[:, 1]).min())})
        assert np.array_equal(passes[-1]["act"], qa.argmax(1))
        return res

    def rec_pre(self, batch, buffer, indices):
        assert "weight" not in batch.get_keys()
        n0 = len(passes)
        b = orig_pre(self, batch, buffer, indices)
        assert len(passes) == n0 + 1                                  # one target pass per batch
        rec.append({"indices": np.array(indices, np.int64), "returns": b.returns.numpy().copy().reshape(-1),
                    "target_act": passes[-1]["act"].copy()})
        return b

    def rec_upd(self, batch):
        stats = orig_upd(self, batch)
        for k in ("loss", "q_loss", "i_loss", "reg_loss"):
            rec[-1][k] = np.array(float(getattr(stats, k)))
        return stats

    DiscreteBCQPolicy.forward, DiscreteBCQ._preprocess_batch, DiscreteBCQ._update_with_batch = rec_fwd, rec_pre, rec_upd
    try:
        for u in range(n_updates):
            with policy_within_training_step(algorithm.policy):
                algorithm.update(buffer=buf, sample_size=batch)
            for k, v in rec[-1].items():
                out[f"u{u}_{k}"] = v
            flat = torch.cat([named[k].detach().reshape(-1) for k in KEYS]).numpy()
            out[f"u{u}_params_strided"] = flat[::STRIDE].copy()
            out[f"u{u}_biases"] = torch.cat([named[k].detach().reshape(-1) for k in KEYS if k.endswith("bias")]).numpy().copy()
            old = dict(old_mod.named_parameters())
            out[f"u{u}_old_params_strided"] = torch.cat([old[k].detach().reshape(-1) for k in OLD_KEYS]).numpy()[::STRIDE].copy()
        opt = algorithm.optim._optim
        st = [opt.state[named[k]] for k in KEYS]
        out["adam_step"] = np.array(int(float(st[0]["step"])))
        out["adam_m_strided"] = torch.cat([s["exp_avg"].reshape(-1) for s in st]).numpy()[::STRIDE].copy()
        out["adam_v_strided"] = torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).numpy()[::STRIDE].copy()
    finally:
        DiscreteBCQPolicy.forward, DiscreteBCQ._preprocess_batch, DiscreteBCQ._update_with_batch = orig_fwd, orig_pre, orig_upd

    assert len(passes) == 2 * n_updates
    changed, dist, gap = [p["changed"] for p in passes], min(p["dist"] for p in passes), min(p["gap"] for p in passes)
    print(f"{tag}: action changed by the mask in {min(changed):.2f} .. {max(changed):.2f} of the rows, smallest threshold "
          f"distance {dist:.3g}, smallest gap of the two best allowed Q values {gap:.3g}")
    if threshold > 0:
        assert min(changed) >= 0.25, changed                        # condition 1
    assert dist >= 1e-3, dist                                       # condition 2
    assert gap >= 1e-3, gap                                         # condition 3
    out["conditions"] = np.array([min(changed), max(changed), dist if np.isfinite(dist) else -1.0, gap], np.float64)

    cfg = dict(gamma=algorithm.gamma, n_step=algorithm.n_step, target_update_freq=algorithm.freq, lr=lr,
               unlikely_action_threshold=threshold, imitation_logits_penalty=algorithm._weight_reg)
    out["cfg_keys"] = np.array(list(cfg.keys()))
    out["cfg_vals"] = np.array(list(cfg.values()), np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"bcq_{tag}.npz"), **out)


def main() -> None:
    geom = dict(E=3, slots=24, steps=30, c=2, h=44, w=36, batch=24, n_updates=3, lr=3e-4)
    gen_bcq("masked", n_act=3, seed=23, gamma=0.95, n_step=3, target_update_freq=2, threshold=0.9, penalty=0.01, **geom)
    gen_bcq("plain", n_act=4, seed=29, gamma=0.9, n_step=1, target_update_freq=1, threshold=0.0, penalty=0.5, **geom)


if __name__ == "__main__":
    main()
