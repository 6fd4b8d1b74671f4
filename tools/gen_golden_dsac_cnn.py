"""TEST INFRASTRUCTURE ONLY - generates tests/golden/dsac_cnn_fixed.npz and tests/golden/dsac_cnn_auto.npz by running the
UNMODIFIED reference (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_dsac_cnn.py

DiscreteSAC.update() (tianshou/algorithm/modelfree/discrete_sac.py) on a DiscreteActor and two DiscreteCritics, single Linear
heads on ONE DQNet(features_only=True, output_dim_added_layer=H), as examples/atari/atari_sac.py builds them, over a synthetic
buffer that stores obs and obs_next:
  "fixed"  a fixed alpha, n_step = 3, a PrioritizedVectorReplayBuffer (importance weights in, priorities out), H = 512;
  "auto"   AutoAlpha, n_step = 1, a plain VectorReplayBuffer, H = 64.
Per update the file holds the sampled indices, the importance weights ("fixed"), batch.returns, the new batch.weight, the five
statistics, log alpha, strided samples of the fourteen live parameters, all biases, and strided samples of `critic_old` and
`critic2_old` (ten tensors each, each with its own trunk copy); once the buffer contents and the manager state, and at the
end the moments of ALL THREE optimizers (each over the trunk and its own head) with their step counts, and AutoAlpha's.  The
initial parameters are not stored: tests/oracle_dsac_cnn.init_params rebuilds them from the seed (checked here against the
reference net, tensor by tensor).  Only data is written; nothing of the reference's program text.

Facts about the reference this script asserts (the engine's design rests on them): each of the three optimizers holds ten
tensors, the shared trunk's eight among them; after every update the trunks of `critic_old` and `critic2_old` are bit-equal.

Three conditions are asserted for every update, so that a fixture cannot pass vacuously:
  1. among the sampled rows at least one has its bootstrap masked (its n-step return does not depend on the target value)
     and at least one has not;
  2. min(q1, q2) on the batch picks each critic in 20 % .. 80 % of the entries;
  3. the mean policy entropy on the batch lies between 10 % and 90 % of log(n_act).
DQNet takes raw pixel values, and the entropy of the freshly initialised actor follows the size of its input: with the sibling
fixtures' sparse frames (6 % of the pixels set, values 0 .. 255) it is all but uniform (0.95 of log A), with dense frames all but
deterministic.  The frames here have a fraction DENSITY of their pixels set to values in 0 .. OBS_MAX, and the sampler is
seeded with seed + SEED_OFFSET (np.random for the prioritized buffer, the buffer's own generator for the plain one).
`python tools/gen_golden_dsac_cnn.py --search` walks GRID = (OBS_MAX, DENSITY) pairs in order and, for each, offsets 0 .. 7,
and prints the first triple at which all conditions hold for both files.  Recorded result: (255, 0.06) fails condition 3 at
0.954 of log A, (255, 0.12) at 0.905; at (255, 0.25) offsets 0 .. 2 sample only rows of one kind in one "auto" update
(condition 1), offset 3 is the first that holds.  At it: "fixed" masks 25 .. 42 % of the rows, picks critic 1 in 67 .. 69 % of
the entries, entropy 0.73 .. 0.88 of log A; "auto" masks 4 .. 17 %, picks critic 1 in 51 .. 58 %, entropy 0.63 .. 0.87 of
log A (the `conditions` array of each file holds them per update).
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

from tianshou.algorithm.modelfree.discrete_sac import DiscreteSAC, DiscreteSACPolicy  # noqa: E402
from tianshou.algorithm.modelfree.sac import AutoAlpha  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.env.atari.atari_network import DQNet  # noqa: E402
from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from oracle import oracle as O  # noqa: E402
from tests import oracle_dsac_cnn as OS  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
KEYS = OS.TIANSHOU_KEYS
SET_KEYS = OS._TRUNK_KEYS + OS._HEAD_KEYS            # one module's ten tensors
STRIDE = 61
OBS_MAX = 255
DENSITY = 0.25
SEED_OFFSET = 3


class ConditionMissed(AssertionError):
    pass


def manager_state(buf) -> dict:
    return {"offset": np.array(buf._extend_offset, np.int64), "last_index": np.array(buf.last_index, np.int64),
            "lengths": np.array(buf._lengths, np.int64),
            "insertion": np.asarray([b._insertion_idx for b in buf.buffers], np.int64)}


def _cat(tensors) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1) for t in tensors]).numpy()


def gen(tag: str, *, prioritized: bool, auto_alpha: bool, E: int, slots: int, steps: int, c: int, h: int, w: int, n_act: int,
        hidden: int, batch: int, n_updates: int, seed: int, actor_lr: float, critic_lr: float, alpha_lr: float, gamma: float,
        tau: float, n_step: int, alpha: float, log_alpha0: float, obs_max: int = OBS_MAX, density: float = DENSITY, offset: int = SEED_OFFSET,
        write: bool = True) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    net = DQNet(c, h, w, action_shape=n_act, features_only=True, output_dim_added_layer=hidden)
    actor = DiscreteActor(preprocess_net=net, action_shape=n_act, softmax_output=False)
    critic1 = DiscreteCritic(preprocess_net=net, last_size=n_act)
    critic2 = DiscreteCritic(preprocess_net=net, last_size=n_act)
    target_entropy = 0.98 * float(np.log(n_act))
    alpha_param = AutoAlpha(target_entropy, log_alpha0, AdamOptimizerFactory(lr=alpha_lr)) if auto_alpha else alpha
    policy = DiscreteSACPolicy(actor=actor, action_space=gym.spaces.Discrete(n_act))
    algorithm = DiscreteSAC(policy=policy, policy_optim=AdamOptimizerFactory(lr=actor_lr), critic=critic1,
                            critic_optim=AdamOptimizerFactory(lr=critic_lr), critic2=critic2,
                            critic2_optim=AdamOptimizerFactory(lr=critic_lr), tau=tau, gamma=gamma, alpha=alpha_param,
                            n_step_return_horizon=n_step)
    named = dict(torch.nn.ModuleList([policy, critic1, critic2]).named_parameters())
    assert list(named.keys()) == KEYS, list(named.keys())
    assert actor.preprocess is critic1.preprocess and actor.preprocess is critic2.preprocess
    live = [named[k] for k in KEYS]
    sets = {"critic1": (algorithm.critic_optim, live[:8] + live[10:12]), "critic2": (algorithm.critic2_optim, live[:8] + live[12:14]),
            "actor": (algorithm.policy_optim, live[:10])}
    for name, (opt, own) in sets.items():                         # the trunk's eight tensors sit in all three optimizers
        held = [p for g in opt._optim.param_groups for p in g["params"]]
        assert len(held) == 10 and {id(p) for p in held} == {id(p) for p in own}, name
    olds = [getattr(m, "module", m) for m in (algorithm.critic_old, algorithm.critic2_old)]
    for m in olds:
        assert list(dict(m.named_parameters()).keys()) == SET_KEYS
    assert olds[0].preprocess is not olds[1].preprocess           # two deep copies: two lagged trunks
    p0 = OS.init_params(c, h, w, n_act, hidden, seed)             # the tests rebuild the initial net from the seed
    for k_ref, k in zip(KEYS, OS.PARAM_ORDER):
        assert torch.equal(named[k_ref], p0[k]), f"oracle init differs from the reference net at {k}"

    if prioritized:
        buf = PrioritizedVectorReplayBuffer(E * slots, E, alpha=0.6, beta=0.4)
    else:
        buf = VectorReplayBuffer(E * slots, E, random_seed=seed + offset)
    frames = rng.integers(0, obs_max + 1, size=(steps + 1, E, c, h, w), dtype=np.uint8)
    frames = np.where(rng.random(frames.shape) < density, frames, 0).astype(np.uint8)
    act = rng.integers(0, n_act, size=(steps, E))
    rew = rng.normal(size=(steps, E)).astype(np.float32)
    term = rng.random((steps, E)) < 0.08
    trunc = (rng.random((steps, E)) < 0.04) & ~term
    for t in range(steps):
        buf.add(Batch(obs=frames[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=frames[t + 1]))
    out: dict[str, np.ndarray] = {}
    out["dims"] = np.array([E, slots, steps, c, h, w, n_act, hidden, batch, n_updates, seed, int(prioritized)])
    out["frames"] = np.asarray(buf.obs, np.uint8)
    out["frames_next"] = np.asarray(buf.obs_next, np.uint8)
    out["act"] = np.asarray(buf.act, np.int64)
    out["rew"] = np.asarray(buf.rew, np.float64)
    out["terminated"] = np.asarray(buf.terminated, bool)
    out["truncated"] = np.asarray(buf.truncated, bool)
    for k, v in manager_state(buf).items():
        out["buf_" + k] = v
    bstate = O.BufferState(out["buf_offset"], out["buf_last_index"], out["buf_lengths"], out["buf_insertion"], out["rew"],
                           out["terminated"], out["truncated"])

    rec: list[dict] = []
    orig_pre, orig_upd = DiscreteSAC._preprocess_batch, DiscreteSAC._update_with_batch

    def rec_pre(self, batch, buffer, indices):
        r = {"indices": np.array(indices, np.int64)}
        if prioritized:
            r["is_weight"] = np.array(batch.weight, np.float64)
        else:
            assert "weight" not in batch.get_keys()
        b = orig_pre(self, batch, buffer, indices)
        r["returns"] = b.returns.detach().numpy().astype(np.float32).reshape(-1).copy()
        rec.append(r)
        return b

    def rec_upd(self, batch):
        with torch.no_grad():                                     # the conditions, on the net the update starts from
            lg, _ = actor(batch.obs)
            q1, q2 = critic1(batch.obs), critic2(batch.obs)
            ent = torch.distributions.Categorical(logits=lg).entropy()
        rec[-1]["cond_entropy"] = np.array(float(ent.mean()) / max(float(np.log(n_act)), 1e-30))
        rec[-1]["cond_pick1"] = np.array(float((q1 < q2).float().mean()))
        stats = orig_upd(self, batch)
        rec[-1]["weight_out"] = batch.weight.detach().numpy().astype(np.float32).copy()
        rec[-1]["stats"] = np.array([stats.actor_loss, stats.critic1_loss, stats.critic2_loss, stats.alpha,
                                     stats.alpha_loss if stats.alpha_loss is not None else 0.0], np.float64)
        return stats

    DiscreteSAC._preprocess_batch, DiscreteSAC._update_with_batch = rec_pre, rec_upd
    try:
        np.random.seed(seed + offset)
        for u in range(n_updates):
            with policy_within_training_step(algorithm.policy):
                algorithm.update(buffer=buf, sample_size=batch)
            r = rec[-1]
            # condition 1: rows whose n-step return does not move with the target value
            r0, _ = O.compute_nstep_return(bstate, r["indices"], lambda after: np.zeros(len(after), np.float32), gamma, n_step)
            r1, _ = O.compute_nstep_return(bstate, r["indices"], lambda after: np.ones(len(after), np.float32), gamma, n_step)
            masked = (np.asarray(r0).reshape(-1) == np.asarray(r1).reshape(-1))
            r["cond_masked"] = np.array(float(masked.mean()))
            if masked.all() or not masked.any():
                raise ConditionMissed(f"{tag} u{u}: bootstrap masks all alike")
            if not 0.2 <= float(r["cond_pick1"]) <= 0.8:
                raise ConditionMissed(f"{tag} u{u}: min(q1, q2) picks critic 1 in {float(r['cond_pick1']):.2f} of the entries")
            if not 0.1 <= float(r["cond_entropy"]) <= 0.9:
                raise ConditionMissed(f"{tag} u{u}: mean entropy {float(r['cond_entropy']):.3f} of log A")
            for k, v in r.items():
                out[f"u{u}_{k}"] = v
            out[f"u{u}_params_strided"] = _cat(live)[::STRIDE].copy()
            out[f"u{u}_biases"] = _cat([named[k] for k in KEYS if k.endswith("bias")]).copy()
            o1, o2 = (dict(m.named_parameters()) for m in olds)
            assert all(torch.equal(o1[k], o2[k]) for k in OS._TRUNK_KEYS), "the two lagged trunks differ"
            out[f"u{u}_critic_old_strided"] = _cat([o1[k] for k in SET_KEYS])[::STRIDE].copy()
            out[f"u{u}_critic2_old_strided"] = _cat([o2[k] for k in SET_KEYS])[::STRIDE].copy()
            out[f"u{u}_log_alpha"] = np.array(float(algorithm.alpha._log_alpha.detach()) if auto_alpha else float(np.log(alpha)))
        for name, (opt, own) in sets.items():
            st = [opt._optim.state[p] for p in own]
            assert all(int(float(s["step"])) == n_updates for s in st)
            out[f"adam_{name}_m_strided"] = _cat([s["exp_avg"] for s in st])[::STRIDE].copy()
            out[f"adam_{name}_v_strided"] = _cat([s["exp_avg_sq"] for s in st])[::STRIDE].copy()
            out[f"adam_{name}_trunk_bias_m"] = _cat([s["exp_avg"] for s in st[1:8:2]]).copy()
        out["adam_step"] = np.array(n_updates)
        if auto_alpha:
            s = algorithm.alpha._optim.state[algorithm.alpha._log_alpha]
            out["alpha_adam"] = np.array([float(s["exp_avg"]), float(s["exp_avg_sq"]), float(s["step"])])
    finally:
        DiscreteSAC._preprocess_batch, DiscreteSAC._update_with_batch = orig_pre, orig_upd

    cond = np.array([[float(r["cond_masked"]), float(r["cond_pick1"]), float(r["cond_entropy"])] for r in rec])
    print(f"{tag}: obs_max {obs_max} density {density} offset {offset}: masked rows {cond[:, 0].min():.2f} .. {cond[:, 0].max():.2f}, critic 1 picked "
          f"{cond[:, 1].min():.2f} .. {cond[:, 1].max():.2f}, entropy / log A {cond[:, 2].min():.3f} .. {cond[:, 2].max():.3f}")
    out["conditions"] = cond
    cfg = dict(gamma=gamma, tau=tau, n_step=n_step, alpha=alpha, auto_alpha=float(auto_alpha), target_entropy=target_entropy,
               log_alpha0=log_alpha0, actor_lr=actor_lr, critic_lr=critic_lr, alpha_lr=alpha_lr, obs_max=obs_max, density=density)
    out["cfg_keys"] = np.array(list(cfg.keys()))
    out["cfg_vals"] = np.array(list(cfg.values()), np.float64)
    if write:
        os.makedirs(OUT, exist_ok=True)
        np.savez_compressed(os.path.join(OUT, f"dsac_cnn_{tag}.npz"), **out)


GEOM = dict(E=3, slots=24, steps=30, c=2, h=44, w=36, batch=24, actor_lr=3e-4, critic_lr=1e-4, alpha_lr=1e-3, tau=0.05)
FILES = {
    "fixed": dict(prioritized=True, auto_alpha=False, n_act=3, hidden=512, seed=41, gamma=0.95, n_step=3, alpha=0.05,
                  log_alpha0=0.0, n_updates=3),
    "auto": dict(prioritized=False, auto_alpha=True, n_act=6, hidden=64, seed=43, gamma=0.9, n_step=1, alpha=0.2,
                 log_alpha0=-1.0, n_updates=4),
}


GRID = ((255, 0.06), (255, 0.12), (255, 0.25), (255, 0.5), (255, 1.0), (128, 1.0), (64, 1.0))       # (OBS_MAX, DENSITY)


def search() -> tuple[int, float, int]:
    for obs_max, density in GRID:
        for off in range(8):
            try:
                for tag, kw in FILES.items():
                    gen(tag, obs_max=obs_max, density=density, offset=off, write=False, **kw, **GEOM)
                return obs_max, density, off
            except ConditionMissed as e:
                print(f"obs_max {obs_max} density {density} offset {off}: {e}")
    raise SystemExit("no (obs_max, density, offset) meets the conditions")


def main() -> None:
    if "--search" in sys.argv:
        print("first (obs_max, density, offset) meeting all conditions:", search())
        return
    for tag, kw in FILES.items():
        gen(tag, **kw, **GEOM)


if __name__ == "__main__":
    main()
