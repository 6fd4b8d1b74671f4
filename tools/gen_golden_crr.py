"""TEST INFRASTRUCTURE ONLY - generates tests/golden/crr_exp.npz and tests/golden/crr_binary.npz by running the
UNMODIFIED reference (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_crr.py

DiscreteCRR.update() (tianshou/algorithm/imitation/discrete_crr.py) on a DiscreteActor and a DiscreteCritic over one
DQNet(features_only=True) trunk, as examples/offline/atari_crr.py builds them, over a synthetic plain VectorReplayBuffer that
stores obs and obs_next: "exp" with lagged networks synced every second update, a small beta and a low ratio_upper_bound, so
that the clamp decides rows; "binary" without lagged networks.  Per update the file holds the sampled indices, the targets
(the very tensor the reference hands to its critic loss), loss / actor_loss / critic_loss / cql_loss, the advantages, strided
parameter samples, all biases and the lagged strided parameters of `actor_old` and `critic_old`; once the buffer contents, the
manager state and the Adam moments at the end.  The initial parameters are not stored: tests/oracle_crr.init_params rebuilds
them from the seed (checked here against the reference net, tensor by tensor).  Only data is written; nothing of the
reference's program text.

Four conditions are asserted, so that a fixture cannot pass vacuously or sit on a knife edge:
  1. "exp": in every update between 20 % and 80 % of the rows have exp(adv / beta) > ratio_upper_bound;
  2. "exp": every row has |exp(adv / beta) - U| >= 1e-3 * U;
  3. "binary": between 20 % and 80 % of the rows have adv > 0, and every |adv| >= 1e-4;
  4. both: among the sampled rows of every update at least one has done > 0 and at least one has not.
The buffer draws its indices from a generator of its own; it is seeded with seed + SEED_OFFSET, the first offset (counted
from 0, the same for both files) at which all four hold: 4 (offsets 0 and 1 sample only unfinished rows in one "exp" update,
2 and 3 clamp more than 80 % of the rows of one).  At it: "exp" clamps 50 .. 67 % of the rows, smallest relative distance
from the bound 2.6e-2; "binary" has adv > 0 in 46 .. 54 % of the rows, smallest |adv| 4.1e-3.
`python tools/gen_golden_crr.py --search` repeats the search.
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
import torch.nn.functional as F  # noqa: E402
import gymnasium as gym  # noqa: E402  (shim stub)

from tianshou.algorithm.imitation.discrete_crr import DiscreteCRR  # noqa: E402
from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou.env.atari.atari_network import DQNet  # noqa: E402
from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from tests import oracle_crr as OC  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
KEYS = OC.TIANSHOU_KEYS
ACTOR_KEYS = [k[len("0.actor."):] for k in KEYS[:10]]         # actor_old: its own trunk + the actor head
CRITIC_KEYS = ACTOR_KEYS[:6] + [k[len("1."):] for k in KEYS[10:]]   # critic_old: its own trunk + the critic head
STRIDE = 61
SEED_OFFSET = 4


class ConditionMissed(AssertionError):
    pass


def manager_state(buf) -> dict:
    return {"offset": np.array(buf._extend_offset, np.int64), "last_index": np.array(buf.last_index, np.int64),
            "lengths": np.array(buf._lengths, np.int64),
            "insertion": np.asarray([b._insertion_idx for b in buf.buffers], np.int64)}


def gen_crr(tag: str, *, E: int, slots: int, steps: int, c: int, h: int, w: int, n_act: int, batch: int, n_updates: int, seed: int,
            lr: float, gamma: float, mode: str, beta: float, ratio_upper_bound: float, min_q_weight: float,
            target_update_freq: int, offset: int = SEED_OFFSET, write: bool = True) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    feature_net = DQNet(c=c, h=h, w=w, action_shape=n_act, features_only=True)
    actor = DiscreteActor(preprocess_net=feature_net, action_shape=n_act, hidden_sizes=[512], softmax_output=False)
    critic = DiscreteCritic(preprocess_net=feature_net, hidden_sizes=[512], last_size=n_act)
    policy = DiscreteActorPolicy(actor=actor, action_space=gym.spaces.Discrete(n_act))
    algorithm = DiscreteCRR(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=lr), gamma=gamma,
                            policy_improvement_mode=mode, ratio_upper_bound=ratio_upper_bound, beta=beta,
                            min_q_weight=min_q_weight, target_update_freq=target_update_freq)
    named = dict(torch.nn.ModuleList([policy, critic]).named_parameters())
    assert list(named.keys()) == KEYS, list(named.keys())
    assert actor.preprocess is critic.preprocess
    assert len(algorithm.optim._optim.param_groups) == 1 and len(algorithm.optim._optim.param_groups[0]["params"]) == 14
    lagged = target_update_freq > 0
    if lagged:
        a_old = getattr(algorithm.actor_old, "module", algorithm.actor_old)
        c_old = getattr(algorithm.critic_old, "module", algorithm.critic_old)
        assert list(dict(a_old.named_parameters()).keys()) == ACTOR_KEYS
        assert list(dict(c_old.named_parameters()).keys()) == CRITIC_KEYS
        assert a_old.preprocess is not c_old.preprocess               # two deep copies: two lagged trunks
    else:
        assert algorithm.actor_old is policy.actor and algorithm.critic_old is critic
    p0 = OC.init_params(c, h, w, n_act, seed)                    # the tests rebuild the initial net from the seed
    for k_ref, k in zip(KEYS, OC.PARAM_ORDER):
        assert torch.equal(named[k_ref], p0[k]), f"oracle init differs from the reference net at {k}"

    buf = VectorReplayBuffer(E * slots, E, random_seed=seed + offset)
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
    orig_pre, orig_upd, orig_mse = DiscreteCRR._preprocess_batch, DiscreteCRR._update_with_batch, F.mse_loss

    def rec_pre(self, batch, buffer, indices):
        assert "weight" not in batch.get_keys()
        b = orig_pre(self, batch, buffer, indices)
        rec.append({"indices": np.array(indices, np.int64), "done": np.asarray(b.done).astype(np.uint8).copy(),
                    "batch_rew": np.asarray(b.rew, np.float64).copy()})
        return b

    def rec_mse(inp, target, *a, **k):
        rec[-1]["target"] = target.detach().numpy().astype(np.float32).reshape(-1).copy()
        return orig_mse(inp, target, *a, **k)

    def rec_upd(self, batch):
        with torch.no_grad():                                     # the advantages of the net the update starts from
            q = critic(batch.obs)
            lg, _ = actor(batch.obs)
            a = torch.as_tensor(np.asarray(batch.act), dtype=torch.int64)
            adv = q.gather(1, a[:, None]).flatten() - (q * torch.softmax(lg, 1)).sum(1)
        rec[-1]["adv"] = adv.numpy().astype(np.float32).copy()
        stats = orig_upd(self, batch)
        for k in ("loss", "actor_loss", "critic_loss", "cql_loss"):
            rec[-1][k] = np.array(float(getattr(stats, k)))
        return stats

    DiscreteCRR._preprocess_batch, DiscreteCRR._update_with_batch, F.mse_loss = rec_pre, rec_upd, rec_mse
    try:
        for u in range(n_updates):
            with policy_within_training_step(algorithm.policy):
                algorithm.update(buffer=buf, sample_size=batch)
            assert "target" in rec[-1]
            for k, v in rec[-1].items():
                out[f"u{u}_{k}"] = v
            flat = torch.cat([named[k].detach().reshape(-1) for k in KEYS]).numpy()
            out[f"u{u}_params_strided"] = flat[::STRIDE].copy()
            out[f"u{u}_biases"] = torch.cat([named[k].detach().reshape(-1) for k in KEYS if k.endswith("bias")]).numpy().copy()
            if lagged:
                ao, co = dict(a_old.named_parameters()), dict(c_old.named_parameters())
                out[f"u{u}_actor_old_strided"] = torch.cat([ao[k].detach().reshape(-1) for k in ACTOR_KEYS]).numpy()[::STRIDE].copy()
                out[f"u{u}_critic_old_strided"] = torch.cat([co[k].detach().reshape(-1) for k in CRITIC_KEYS]).numpy()[::STRIDE].copy()
        opt = algorithm.optim._optim
        st = [opt.state[named[k]] for k in KEYS]
        out["adam_step"] = np.array(int(float(st[0]["step"])))
        out["adam_m_strided"] = torch.cat([s["exp_avg"].reshape(-1) for s in st]).numpy()[::STRIDE].copy()
        out["adam_v_strided"] = torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).numpy()[::STRIDE].copy()
    finally:
        DiscreteCRR._preprocess_batch, DiscreteCRR._update_with_batch, F.mse_loss = orig_pre, orig_upd, orig_mse

    assert algorithm._iter == n_updates
    cond = []
    for u, r in enumerate(rec):
        adv = r["adv"]
        if not (r["done"] > 0).any() or (r["done"] > 0).all():                                   # condition 4
            raise ConditionMissed(f"{tag} u{u}: done flags all alike")
        if mode == "exp":
            e = np.exp((adv / np.float32(beta)).astype(np.float32)).astype(np.float64)
            frac, dist = float((e > ratio_upper_bound).mean()), float((np.abs(e - ratio_upper_bound) / ratio_upper_bound).min())
            if not 0.2 <= frac <= 0.8:                                                           # condition 1
                raise ConditionMissed(f"{tag} u{u}: {frac:.2f} of the rows clamped")
            if dist < 1e-3:                                                                      # condition 2
                raise ConditionMissed(f"{tag} u{u}: relative distance from the bound {dist:.3g}")
        else:
            frac, dist = float((adv > 0).mean()), float(np.abs(adv).min())
            if not 0.2 <= frac <= 0.8 or dist < 1e-4:                                            # condition 3
                raise ConditionMissed(f"{tag} u{u}: {frac:.2f} of the rows positive, smallest |adv| {dist:.3g}")
        cond.append((frac, dist))
    print(f"{tag}: offset {offset}: rows {'clamped' if mode == 'exp' else 'with adv > 0'} "
          f"{min(f for f, _ in cond):.2f} .. {max(f for f, _ in cond):.2f}, smallest distance {min(d for _, d in cond):.3g}")
    out["conditions"] = np.array(cond, np.float64)

    cfg = dict(gamma=gamma, mode=OC.MODES.index(mode), beta=beta, ratio_upper_bound=ratio_upper_bound,
               min_q_weight=min_q_weight, target_update_freq=target_update_freq, lr=lr)
    out["cfg_keys"] = np.array(list(cfg.keys()))
    out["cfg_vals"] = np.array(list(cfg.values()), np.float64)
    if write:
        os.makedirs(OUT, exist_ok=True)
        np.savez_compressed(os.path.join(OUT, f"crr_{tag}.npz"), **out)


GEOM = dict(E=3, slots=24, steps=30, c=2, h=44, w=36, batch=24, lr=3e-4)
FILES = {
    "exp": dict(n_act=3, seed=31, gamma=0.95, mode="exp", beta=0.05, ratio_upper_bound=1.5, min_q_weight=10.0,
                target_update_freq=2, n_updates=5),
    "binary": dict(n_act=4, seed=37, gamma=0.9, mode="binary", beta=1.0, ratio_upper_bound=20.0, min_q_weight=2.5,
                   target_update_freq=0, n_updates=3),
}


def search(limit: int = 64) -> int:
    for off in range(limit):
        try:
            for tag, kw in FILES.items():
                gen_crr(tag, offset=off, write=False, **kw, **GEOM)
            return off
        except ConditionMissed as e:
            print(f"offset {off}: {e}")
    raise SystemExit("no offset meets the four conditions")


def main() -> None:
    if "--search" in sys.argv:
        print("first offset meeting all conditions:", search())
        return
    for tag, kw in FILES.items():
        gen_crr(tag, **kw, **GEOM)


if __name__ == "__main__":
    main()
