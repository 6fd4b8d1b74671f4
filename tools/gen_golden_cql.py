"""TEST INFRASTRUCTURE ONLY - generates tests/golden/cql_calibrated.npz and tests/golden/cql_plain.npz by running the
UNMODIFIED reference on the CPU (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_cql.py

CQL.update() (tianshou/algorithm/imitation/cql.py) over a synthetic replay buffer:
  "calibrated": the setup of examples/offline/d4rl_cql.py -- Net[256, 256] ReLU, AutoAlpha, the Lagrange multiplier and the
                Cal-QL calibration on, R = 10, the default min_action / max_action (uniform_(1, 1): every random action is 1.0);
  "plain":      three nn.Tanh layers of unequal widths, actor and critics differing, fixed alpha, no multiplier, no calibration,
                T = 0.7, cql_weight = 5, min_action = +1.0 (U(-1, 1) random actions), R = 3.
On the CPU the reference's `cql_log_alpha.to(device)` is the optimizer's leaf itself, so the multiplier learns (on a cuda
device the copy is never stepped).  Per update the file holds the sampled indices, the five random tensors in draw order (rsample
eps of the actor loss and of the target, random_actions, rsample eps of pi(tmp_obs) and of pi(tmp_obs_next)), the seven
statistics, both critics' gradient norms before clipping, cql_log_alpha and every 61st element of each network and lagged
network; once the buffer with its calibration_returns and every 61st element of the Adam moments at the end.  The initial
parameters are not stored: oracle_sac.init_sac_params rebuilds them from the seed (checked here against the reference nets,
tensor by tensor).  Only data is written; nothing of the reference's program text.
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
import torch.distributions.normal as tdn  # noqa: E402
from torch import nn  # noqa: E402
import gymnasium as gym  # noqa: E402  (shim stub)

from tianshou.algorithm.imitation.cql import CQL  # noqa: E402
from tianshou.algorithm.modelfree.sac import AutoAlpha, SACPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from oracle import oracle_sac as OS  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
CLIP_COEFS: dict[str, list[float]] = {}


def gen_cql(tag: str, *, E: int, slots: int, steps: int, obs_dim: int, act_dim: int, batch: int, n_updates: int, seed: int,
            hidden, activation, auto_alpha: bool, alpha: float, with_lagrange: bool, calibrated: bool, temperature: float,
            cql_weight: float, min_action: float, max_action: float, R: int, max_grad_norm: float, lagrange_threshold: float = 10.0,
            actor_lr: float = 1e-4, critic_lr: float = 3e-4, alpha_lr: float = 1e-4, cql_alpha_lr: float = 3e-4, tau: float = 0.005,
            gamma: float = 0.99) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    sa_, sc_ = OS.layer_sizes(hidden)
    AK, CK = OS.trunk_keys(len(sa_), ("mu", "sigma")), OS.trunk_keys(len(sc_), ("last",))
    net_a = Net(state_shape=(obs_dim,), hidden_sizes=list(sa_), activation=activation)
    actor = ContinuousActorProbabilistic(preprocess_net=net_a, action_shape=(act_dim,), unbounded=True, conditioned_sigma=True)
    mk_net = lambda: Net(state_shape=(obs_dim,), action_shape=(act_dim,), hidden_sizes=list(sc_), concat=True,  # noqa: E731
                         activation=activation)
    n1, n2 = mk_net(), mk_net()
    critic1, critic2 = ContinuousCritic(preprocess_net=n1), ContinuousCritic(preprocess_net=n2)
    p0 = OS.init_sac_params(obs_dim, act_dim, seed, (sa_, sc_))             # the tests rebuild the initial nets from the seed
    for pd, order, mod, keys in ((p0[0], OS.actor_order(len(sa_)), actor, AK), (p0[1], OS.critic_order(len(sc_)), critic1, CK),
                                 (p0[2], OS.critic_order(len(sc_)), critic2, CK)):
        sd = mod.state_dict()
        assert list(sd.keys()) == keys, list(sd.keys())
        for k_ref, k in zip(keys, order):
            assert torch.equal(sd[k_ref], pd[k]), f"oracle init differs from the reference at {k}"
    policy = SACPolicy(actor=actor, action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(act_dim,)))
    al = AutoAlpha(float(-act_dim), 0.0, AdamOptimizerFactory(lr=alpha_lr)) if auto_alpha else alpha
    algorithm = CQL(policy=policy, policy_optim=AdamOptimizerFactory(lr=actor_lr), critic=critic1,
                    critic_optim=AdamOptimizerFactory(lr=critic_lr), critic2=critic2,
                    critic2_optim=AdamOptimizerFactory(lr=critic_lr), cql_alpha_lr=cql_alpha_lr, cql_weight=cql_weight, tau=tau,
                    gamma=gamma, alpha=al, temperature=temperature, with_lagrange=with_lagrange,
                    lagrange_threshold=lagrange_threshold, min_action=min_action, max_action=max_action, num_repeat_actions=R,
                    max_grad_norm=max_grad_norm, calibrated=calibrated)
    buf = VectorReplayBuffer(E * slots, E)
    obs = rng.normal(size=(steps + 1, E, obs_dim)).astype(np.float32)
    act = rng.uniform(-1, 1, size=(steps, E, act_dim)).astype(np.float32)
    rew = rng.normal(size=(steps, E)).astype(np.float32)
    term = rng.random((steps, E)) < 0.05
    trunc = (rng.random((steps, E)) < 0.03) & ~term
    for t in range(steps):
        buf.add(Batch(obs=obs[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=obs[t + 1]))
    # (steps == slots: process_buffer stores one return per FILLED slot, and sampling indexes it by buffer position)
    buf = algorithm.process_buffer(buf)                                       # cql.py:244-266: calibration_returns, once
    out: dict[str, np.ndarray] = {"dims": np.array([E, slots, steps, obs_dim, act_dim, batch, n_updates, seed, R]),
                                  "hidden_actor": np.array(sa_, np.int64), "hidden_critic": np.array(sc_, np.int64)}
    for k2 in ("obs", "obs_next", "act"):
        out[k2] = np.asarray(getattr(buf, k2), np.float32)
    out["rew"], out["terminated"], out["truncated"] = (np.asarray(buf.rew, np.float64), np.asarray(buf.terminated, bool),
                                                       np.asarray(buf.truncated, bool))
    out["done"] = np.asarray(buf.done, bool)
    if calibrated:
        out["calibration_returns"] = np.asarray(buf._meta.calibration_returns, np.float64)

    draws: list[tuple[str, np.ndarray]] = []
    norms: list[float] = []
    rec: list[dict] = []
    orig_sn, orig_rand, orig_clip = tdn._standard_normal, CQL._calc_random_values, nn.utils.clip_grad_norm_
    orig_upd = CQL._update_with_batch

    def rec_sn(shape, dtype, device):
        e = orig_sn(shape, dtype, device)
        draws.append(("normal", e.numpy().copy()))
        return e

    def rec_rand(self, obs_, act_):
        draws.append(("random", act_.detach().numpy().copy()))
        return orig_rand(self, obs_, act_)

    def rec_clip(parameters, max_norm, *a, **k):
        n = orig_clip(parameters, max_norm, *a, **k)
        norms.append(float(n))
        return n

    def rec_upd(self, batch):
        rec.append({"done": np.asarray(batch.done).copy()})
        return orig_upd(self, batch)

    tdn._standard_normal, CQL._calc_random_values, nn.utils.clip_grad_norm_ = rec_sn, rec_rand, rec_clip
    CQL._update_with_batch = rec_upd
    orig_sample = buf.sample_indices
    sampled: list[np.ndarray] = []

    def rec_sample(n):
        i = orig_sample(n)
        sampled.append(np.array(i, np.int64))
        return i

    buf.sample_indices = rec_sample
    coefs = []
    try:
        np.random.seed(seed + 7)
        for u in range(n_updates):
            d0, g0 = len(draws), len(norms)
            with policy_within_training_step(algorithm.policy):
                stats = algorithm.update(buffer=buf, sample_size=batch)
            kinds = [k for k, _ in draws[d0:]]
            # the random actions are drawn BEFORE the two repeated rsamples (cql.py:303-317) and recorded when they are used (:319)
            assert kinds == ["normal", "normal", "normal", "normal", "random"], kinds
            d = [v for _, v in draws[d0:]]
            out[f"u{u}_noise_actor"], out[f"u{u}_noise_next"] = d[0], d[1]
            out[f"u{u}_random_act"], out[f"u{u}_noise_rep_cur"], out[f"u{u}_noise_rep_next"] = d[4], d[2], d[3]
            assert d[0].shape == (batch, act_dim) and d[2].shape == (batch * R, act_dim) and d[4].shape == (batch * R, act_dim)
            assert len(norms) - g0 == 2
            out[f"u{u}_grad_norms"] = np.array(norms[g0:], np.float64)
            coefs += [min(1.0, max_grad_norm / (n + 1e-6)) for n in norms[g0:]]
            out[f"u{u}_indices"] = sampled[-1]
            assert np.array_equal(rec[-1]["done"], np.asarray(buf.done)[sampled[-1]])
            nan = lambda v: np.nan if v is None else v  # noqa: E731
            out[f"u{u}_stats"] = np.array([stats.actor_loss, stats.critic1_loss, stats.critic2_loss, nan(stats.alpha),
                                           nan(stats.alpha_loss), nan(stats.cql_alpha), nan(stats.cql_alpha_loss)], np.float64)
            out[f"u{u}_cql_log_alpha"] = algorithm.cql_log_alpha.detach().numpy().copy()
            for name, mod, keys in (("actor", actor, AK), ("critic1", critic1, CK), ("critic2", critic2, CK),
                                    ("critic1_old", algorithm.critic_old.module, CK),
                                    ("critic2_old", algorithm.critic2_old.module, CK)):
                sd = mod.state_dict()
                out[f"u{u}_{name}"] = torch.cat([sd[k2].reshape(-1) for k2 in keys]).numpy()[::61].copy()
        for name, mod, keys, optim in (("actor", actor, AK, algorithm.policy_optim), ("critic1", critic1, CK, algorithm.critic_optim),
                                       ("critic2", critic2, CK, algorithm.critic2_optim)):
            params = dict(mod.named_parameters())
            st = [optim._optim.state[params[k]] for k in keys]
            out[f"adam_step_{name}"] = np.array(int(float(st[0]["step"])))
            out[f"adam_m_{name}"] = torch.cat([s["exp_avg"].reshape(-1) for s in st]).numpy()[::61].copy()
            out[f"adam_v_{name}"] = torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).numpy()[::61].copy()
        if with_lagrange:
            s = algorithm.cql_alpha_optim.state[algorithm.cql_alpha_optim.param_groups[0]["params"][0]]
            out["adam_cql_alpha"] = np.array([float(s["step"]), float(s["exp_avg"]), float(s["exp_avg_sq"])], np.float64)
    finally:
        tdn._standard_normal, CQL._calc_random_values, nn.utils.clip_grad_norm_ = orig_sn, orig_rand, orig_clip
        CQL._update_with_batch = orig_upd
    CLIP_COEFS[tag] = coefs
    cfg = dict(gamma=gamma, tau=tau, alpha=alpha, auto_alpha=float(auto_alpha), target_entropy=float(-act_dim), log_alpha0=0.0,
               actor_lr=actor_lr, critic_lr=critic_lr, alpha_lr=alpha_lr, cql_alpha_lr=cql_alpha_lr, cql_weight=cql_weight,
               temperature=temperature, with_lagrange=float(with_lagrange), lagrange_threshold=lagrange_threshold,
               min_action=min_action, max_action=max_action, num_repeat_actions=float(R), alpha_min=algorithm.alpha_min,
               alpha_max=algorithm.alpha_max, max_grad_norm=max_grad_norm, calibrated=float(calibrated),
               **({"tanh_trunks": 1.0} if activation is nn.Tanh else {}))
    out["cfg_keys"], out["cfg_vals"] = np.array(list(cfg.keys())), np.array(list(cfg.values()), np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"cql_{tag}.npz"), **out)


def main() -> None:
    gen_cql("calibrated", E=4, slots=32, steps=32, obs_dim=17, act_dim=6, batch=48, n_updates=3, seed=61,
            hidden=((256, 256), (256, 256)), activation=nn.ReLU, auto_alpha=True, alpha=0.2, with_lagrange=True, calibrated=True,
            temperature=1.0, cql_weight=1.0, min_action=-1.0, max_action=1.0, R=10, max_grad_norm=1.0)
    gen_cql("plain", E=4, slots=32, steps=32, obs_dim=23, act_dim=5, batch=32, n_updates=4, seed=62,
            hidden=((64, 48, 32), (40, 72, 56)), activation=nn.Tanh, auto_alpha=False, alpha=0.15, with_lagrange=False,
            calibrated=False, temperature=0.7, cql_weight=5.0, min_action=1.0, max_action=1.0, R=3, max_grad_norm=50.0, tau=0.01,
            gamma=0.97)
    # the clip must bite in one file and be inactive (coefficient exactly 1) in the other, so both branches are pinned
    assert any(c < 1.0 for c in CLIP_COEFS["calibrated"]), CLIP_COEFS
    assert any(c == 1.0 for c in CLIP_COEFS["plain"]), CLIP_COEFS


if __name__ == "__main__":
    main()
