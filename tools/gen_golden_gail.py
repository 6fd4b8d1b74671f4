"""TEST INFRASTRUCTURE ONLY - generates tests/golden/gail_mujoco.npz and tests/golden/gail_odd.npz by running the UNMODIFIED
reference (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_gail.py

GAIL.update() (tianshou/algorithm/imitation/gail.py) twice in a row on a synthetic rollout buffer and a synthetic expert buffer:
"mujoco" -- the networks of examples/inverse/irl_gail.py (obs 17, act 6, all three nets Net[64, 64] tanh), 4 envs x 32 steps,
disc_update_num 2, PPO minibatch 64, repeat 2; "odd" -- obs 5, act 3, a discriminator on three ReLU layers [48, 80, 32], actor
and critic on other trunks, 2 envs x 19 steps (N = 38) with disc_update_num 10 (bsz 3, 12 steps, the last one 5 policy rows
against 3 expert rows), an expert buffer smaller than the rollout, max_grad_norm on both optimizers.
Per update the file holds the split permutation, the expert indices of every step, the float32 rewards, v_s / returns /
advantages / logp_old, the per-step {disc_loss, acc_pi, acc_exp}, the PPO losses and permutations, every 7th element of the
discriminator after the discriminator phase and of all three networks after the update; at the end every 7th element of the
optimizer moments.  The initial parameters are stored in full, as the ppo_net_* fixtures do.  Only data is written; nothing of
the reference's program text.
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
from torch import nn  # noqa: E402
from torch.distributions import Independent, Normal  # noqa: E402
import gymnasium as gym  # noqa: E402  (shim stub)

from tianshou.algorithm.imitation.gail import GAIL  # noqa: E402
from tianshou.algorithm.modelfree.ppo import PPO  # noqa: E402
from tianshou.algorithm.modelfree.reinforce import ProbabilisticActorPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, ReplayBuffer, SequenceSummaryStats, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import ActorCritic, Net  # noqa: E402
from tianshou.utils.net.continuous import ContinuousActorProbabilistic, ContinuousCritic  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
STRIDE = 7


def tensors(mod, head):
    lin = [m for m in mod.preprocess.model.model if isinstance(m, nn.Linear)] + [m for m in head.modules() if isinstance(m, nn.Linear)]
    return [p for m in lin for p in (m.weight, m.bias)]


def strided(ts) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1) for t in ts]).numpy()[::STRIDE].copy()


def gen_gail(tag: str, *, E: int, T: int, obs_dim: int, act_dim: int, hidden_a, hidden_c, hidden_d, activation, disc_activation,
             disc_update_num: int, batch_size: int, repeat: int, n_expert: int, expert_seed: int, seed: int, n_updates: int, lr: float,
             disc_lr: float, disc_max_grad_norm, **ppo_kwargs) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    N = E * T
    actor = ContinuousActorProbabilistic(preprocess_net=Net(state_shape=(obs_dim,), hidden_sizes=list(hidden_a), activation=activation),
                                         action_shape=(act_dim,), unbounded=True)
    critic = ContinuousCritic(preprocess_net=Net(state_shape=(obs_dim,), hidden_sizes=list(hidden_c), activation=activation))
    disc = ContinuousCritic(preprocess_net=Net(state_shape=(obs_dim,), action_shape=(act_dim,), hidden_sizes=list(hidden_d),
                                               activation=disc_activation, concat=True))
    torch.nn.init.constant_(actor.sigma_param, -0.5)
    for m in list(ActorCritic(actor, critic).modules()) + list(disc.modules()):
        if isinstance(m, nn.Linear):
            nn.init.orthogonal_(m.weight, gain=np.sqrt(2))
            nn.init.normal_(m.bias, std=0.1)

    def dist(loc_scale):
        loc, scale = loc_scale
        return Independent(Normal(loc, scale), 1)

    policy = ProbabilisticActorPolicy(actor=actor, dist_fn=dist, action_scaling=True, action_bound_method="clip",
                                      action_space=gym.spaces.Box(low=-1.0, high=1.0, shape=(act_dim,)))
    expert = ReplayBuffer(n_expert, random_seed=expert_seed)
    e_obs = (rng.normal(size=(n_expert + 1, obs_dim)) + 0.4).astype(np.float32)
    e_act = np.tanh(rng.normal(size=(n_expert, act_dim))).astype(np.float32)
    for t in range(n_expert):
        expert.add(Batch(obs=e_obs[t], act=e_act[t], rew=0.0, terminated=False, truncated=False, obs_next=e_obs[t + 1]))
    algorithm = GAIL(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=lr), expert_buffer=expert, disc_net=disc,
                     disc_optim=AdamOptimizerFactory(lr=disc_lr), disc_update_num=disc_update_num, **ppo_kwargs)
    algorithm.disc_optim._max_grad_norm = disc_max_grad_norm          # (what Algorithm._create_optimizer's max_grad_norm sets)
    a_par, c_par, d_par = tensors(actor, actor.mu) + [actor.sigma_param], tensors(critic, critic.last), tensors(disc, disc.last)
    act_id = {nn.Tanh: 0, nn.ReLU: 1, None: 2}
    out: dict[str, np.ndarray] = {
        "dims": np.array([E, T, obs_dim, act_dim, batch_size, repeat, disc_update_num, n_expert, expert_seed, seed, n_updates, STRIDE]),
        "hidden_a": np.array(hidden_a), "hidden_c": np.array(hidden_c), "hidden_d": np.array(hidden_d),
        "activation": np.array(act_id[activation]), "disc_activation": np.array(act_id[disc_activation]),
        "expert_obs": np.asarray(expert.obs, np.float32), "expert_act": np.asarray(expert.act, np.float32)}
    for name, par in (("a", a_par), ("c", c_par), ("d", d_par)):
        for i, t in enumerate(par):
            out[f"{name}{i}_0"] = t.detach().numpy().copy()

    perms, seqs, draws, pre, disc_after = [], [], [], {}, []
    orig_perm, orig_from = np.random.permutation, SequenceSummaryStats.from_sequence.__func__
    orig_pre, orig_ppo_upd, orig_si = GAIL._preprocess_batch, PPO._update_with_batch, ReplayBuffer.sample_indices

    def rec_perm(n):
        q = orig_perm(n)
        perms.append(np.asarray(q, np.int64))
        return q

    def rec_from(c_, seq):
        seqs.append(np.asarray(seq, np.float64))
        return orig_from(c_, seq)

    def rec_si(self, batch_size):
        idx = orig_si(self, batch_size)
        if self is expert:
            draws.append(np.asarray(idx, np.int64))
        return idx

    def rec_pre(self, batch, buffer, indices):
        b = orig_pre(self, batch, buffer, indices)
        assert b.rew.dtype == np.float32
        pre.update(rew=np.asarray(b.rew).copy(), v_s=b.v_s.numpy().copy(), returns=b.returns.numpy().copy(), adv=b.adv.numpy().copy(),
                   logp_old=b.logp_old.numpy().copy(), indices=np.asarray(indices, np.int64))
        return b

    def rec_ppo_upd(self, batch, batch_size_, repeat_):
        disc_after.append(strided(d_par))                          # the discriminator phase is over (gail.py:236-237)
        return orig_ppo_upd(self, batch, batch_size_, repeat_)

    np.random.permutation, SequenceSummaryStats.from_sequence = rec_perm, classmethod(rec_from)
    GAIL._preprocess_batch, PPO._update_with_batch, ReplayBuffer.sample_indices = rec_pre, rec_ppo_upd, rec_si
    try:
        buf = VectorReplayBuffer(N, E)
        obs = rng.normal(size=(T + 1, E, obs_dim)).astype(np.float32)
        act = rng.normal(size=(T, E, act_dim)).astype(np.float32)
        rew = rng.normal(size=(T, E)).astype(np.float32)
        term = rng.random((T, E)) < 0.05
        trunc = np.zeros((T, E), bool)
        for t in range(T):
            buf.add(Batch(obs=obs[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=obs[t + 1]))
        for k in ("obs", "obs_next", "act"):
            out[k] = np.asarray(getattr(buf, k), np.float32)
        out["rew"] = np.asarray(buf.rew, np.float64)
        out["terminated"], out["truncated"] = np.asarray(buf.terminated, bool), np.asarray(buf.truncated, bool)
        np.random.seed(seed + 100)
        bsz = N // disc_update_num
        steps = N // bsz
        for u in range(n_updates):
            p0, s0, d0 = len(perms), len(seqs), len(draws)
            with policy_within_training_step(algorithm.policy):
                stats = algorithm.update(buffer=buf, batch_size=batch_size, repeat=repeat)
            assert len(perms) - p0 == 1 + repeat and len(seqs) - s0 == 7 and len(draws) - d0 == steps
            out[f"u{u}_split_perm"] = perms[p0]
            out[f"u{u}_perms"] = np.stack(perms[p0 + 1:])
            out[f"u{u}_exp_index"] = np.stack(draws[d0:])
            assert out[f"u{u}_exp_index"].shape == (steps, bsz)
            out[f"u{u}_losses"] = np.stack(seqs[s0:s0 + 4], axis=1)       # loss, clip loss, vf loss, entropy loss (ppo.py:218-222)
            out[f"u{u}_disc_stats"] = np.stack(seqs[s0 + 4:s0 + 7], axis=1)  # disc_loss, acc_pi, acc_exp per step (gail.py:239-241)
            assert out[f"u{u}_disc_stats"].shape == (steps, 3)
            out[f"u{u}_gradient_steps"] = np.array(stats.gradient_steps)
            for k, v in pre.items():
                out[f"u{u}_pre_{k}"] = v
            out[f"u{u}_disc_mid"] = disc_after[-1]
            out[f"u{u}_a"], out[f"u{u}_c"], out[f"u{u}_d"] = strided(a_par), strided(c_par), strided(d_par)
            out[f"u{u}_ret_rms"] = np.array([algorithm.ret_rms.mean, algorithm.ret_rms.var, algorithm.ret_rms.count], np.float64)
    finally:
        np.random.permutation, SequenceSummaryStats.from_sequence = orig_perm, classmethod(orig_from)
        GAIL._preprocess_batch, PPO._update_with_batch, ReplayBuffer.sample_indices = orig_pre, orig_ppo_upd, orig_si
    for name, opt, par in (("ac", algorithm.optim._optim, a_par + c_par), ("d", algorithm.disc_optim._optim, d_par)):
        out[f"adam_step_{name}"] = np.array(int(float(opt.state[par[0]]["step"])))
        out[f"adam_m_{name}"] = strided([opt.state[p]["exp_avg"] for p in par])
        out[f"adam_v_{name}"] = strided([opt.state[p]["exp_avg_sq"] for p in par])
    cfg = dict(gamma=algorithm.gamma, gae_lambda=algorithm.gae_lambda, eps_clip=algorithm.eps_clip, dual_clip=algorithm.dual_clip or 0.0,
               value_clip=float(algorithm.value_clip), advantage_normalization=float(algorithm.advantage_normalization),
               vf_coef=algorithm.vf_coef, ent_coef=algorithm.ent_coef, max_grad_norm=algorithm.optim._max_grad_norm or 0.0,
               return_scaling=float(algorithm.return_scaling), lr=lr, disc_lr=disc_lr, disc_max_grad_norm=disc_max_grad_norm or 0.0)
    out["cfg_keys"], out["cfg_vals"] = np.array(list(cfg.keys())), np.array(list(cfg.values()), np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"gail_{tag}.npz"), **out)


def main() -> None:
    gen_gail("mujoco", E=4, T=32, obs_dim=17, act_dim=6, hidden_a=[64, 64], hidden_c=[64, 64], hidden_d=[64, 64], activation=nn.Tanh,
             disc_activation=nn.Tanh, disc_update_num=2, batch_size=64, repeat=2, n_expert=200, expert_seed=42, seed=61, n_updates=2,
             lr=3e-4, disc_lr=1e-3, disc_max_grad_norm=None, eps_clip=0.2, vf_coef=0.25, ent_coef=0.001, max_grad_norm=None,
             value_clip=False, advantage_normalization=False, return_scaling=True, gae_lambda=0.95, gamma=0.99)
    gen_gail("odd", E=2, T=19, obs_dim=5, act_dim=3, hidden_a=[40, 24], hidden_c=[56], hidden_d=[48, 80, 32], activation=nn.Tanh,
             disc_activation=nn.ReLU, disc_update_num=10, batch_size=16, repeat=2, n_expert=20, expert_seed=7, seed=62, n_updates=2,
             lr=1e-3, disc_lr=2e-3, disc_max_grad_norm=0.5, eps_clip=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5,
             value_clip=True, advantage_normalization=True, return_scaling=False, gae_lambda=0.9, gamma=0.98)


if __name__ == "__main__":
    main()
