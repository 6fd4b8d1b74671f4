"""TEST INFRASTRUCTURE ONLY - generates tests/golden/td3bc_offline.npz and tests/golden/td3bc_per_tanh.npz by running the
UNMODIFIED reference (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_td3bc.py

TD3BC.update() (tianshou/algorithm/imitation/td3_bc.py) on the networks of examples/offline/d4rl_td3_bc.py over a synthetic
replay buffer: the offline case, a plain VectorReplayBuffer without weights on Net[256, 256] ReLU with the delayed actor
("offline"), and a PrioritizedVectorReplayBuffer with 3-step returns on three nn.Tanh layers of unequal widths, actor and
critics differing, max_action 1.5 and an actor step at every update ("per_tanh").  Per update the file holds the sampled
indices, the PER weights, new priorities and sum-tree (prioritized buffer only), TD3's torch.randn smoothing noise, the n-step returns,
the three statistics and every 61st element of each network and lagged network (the stride of td3_*.npz); once the buffer
contents, the manager state and every 61st element of the Adam moments at the end.  The initial parameters are not stored:
oracle_sac.init_td3_params rebuilds them from the seed (checked here against the reference nets, tensor by tensor).  Only data
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
from torch import nn  # noqa: E402
import gymnasium as gym  # noqa: E402  (shim stub)

from tianshou.algorithm.imitation.td3_bc import TD3BC  # noqa: E402
from tianshou.algorithm.modelfree.ddpg import ContinuousDeterministicPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
from tianshou.utils.net.continuous import ContinuousActorDeterministic, ContinuousCritic  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from oracle import oracle_sac as OS  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")


def manager_state(buf) -> dict:
    return {"offset": np.array(buf._extend_offset, np.int64), "last_index": np.array(buf.last_index, np.int64),
            "lengths": np.array(buf._lengths, np.int64),
            "insertion": np.asarray([b._insertion_idx for b in buf.buffers], np.int64)}


def gen_td3bc(tag: str, *, prioritized: bool, E: int, slots: int, steps: int, obs_dim: int, act_dim: int, batch: int,
              n_updates: int, seed: int, hidden, activation, max_action: float, alpha: float, update_actor_freq: int, n_step: int,
              actor_lr: float, critic_lr: float, tau: float, gamma: float, policy_noise: float = 0.2,
              noise_clip: float = 0.5) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    sa_, sc_ = OS.layer_sizes(hidden)
    AK, CK = OS.trunk_keys(len(sa_), ("last",)), OS.trunk_keys(len(sc_), ("last",))
    AO, CO = OS.det_actor_order(len(sa_)), OS.critic_order(len(sc_))
    actor = ContinuousActorDeterministic(preprocess_net=Net(state_shape=(obs_dim,), hidden_sizes=list(sa_), activation=activation),
                                         action_shape=(act_dim,), max_action=max_action)
    mk_net = lambda: Net(state_shape=(obs_dim,), action_shape=(act_dim,), hidden_sizes=list(sc_), concat=True,  # noqa: E731
                         activation=activation)
    n1, n2 = mk_net(), mk_net()
    critic1, critic2 = ContinuousCritic(preprocess_net=n1), ContinuousCritic(preprocess_net=n2)
    p0 = OS.init_td3_params(obs_dim, act_dim, seed, True, (sa_, sc_))        # the tests rebuild the initial nets from the seed
    for pd, order, mod, keys in ((p0[0], AO, actor, AK), (p0[1], CO, critic1, CK), (p0[2], CO, critic2, CK)):
        sd = mod.state_dict()
        assert list(sd.keys()) == keys, list(sd.keys())
        for k_ref, k in zip(keys, order):
            assert torch.equal(sd[k_ref], pd[k]), f"oracle init differs from the reference at {k}"
    space = gym.spaces.Box(low=-max_action, high=max_action, shape=(act_dim,))
    policy = ContinuousDeterministicPolicy(actor=actor, action_space=space, exploration_noise=None)
    algorithm = TD3BC(policy=policy, policy_optim=AdamOptimizerFactory(lr=actor_lr), critic=critic1,
                      critic_optim=AdamOptimizerFactory(lr=critic_lr), critic2=critic2,
                      critic2_optim=AdamOptimizerFactory(lr=critic_lr), tau=tau, gamma=gamma, policy_noise=policy_noise,
                      update_actor_freq=update_actor_freq, noise_clip=noise_clip, alpha=alpha, n_step_return_horizon=n_step)
    if prioritized:
        buf = PrioritizedVectorReplayBuffer(E * slots, E, alpha=0.6, beta=0.4)
    else:
        buf = VectorReplayBuffer(E * slots, E)
    obs = rng.normal(size=(steps + 1, E, obs_dim)).astype(np.float32)
    act = rng.uniform(-max_action, max_action, size=(steps, E, act_dim)).astype(np.float32)
    rew = rng.normal(size=(steps, E)).astype(np.float32)
    term = rng.random((steps, E)) < 0.05
    trunc = (rng.random((steps, E)) < 0.03) & ~term
    for t in range(steps):
        buf.add(Batch(obs=obs[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=obs[t + 1]))
    out: dict[str, np.ndarray] = {
        "dims": np.array([E, slots, steps, obs_dim, act_dim, batch, n_updates, seed, int(prioritized), n_step]),
        "hidden_actor": np.array(sa_, np.int64), "hidden_critic": np.array(sc_, np.int64)}
    for k2 in ("obs", "obs_next", "act"):
        out[k2] = np.asarray(getattr(buf, k2), np.float32)
    out["rew"], out["terminated"], out["truncated"] = (np.asarray(buf.rew, np.float64), np.asarray(buf.terminated, bool),
                                                       np.asarray(buf.truncated, bool))
    for k2, v in manager_state(buf).items():
        out["buf_" + k2] = v
    if prioritized:
        out["tree0"] = np.asarray(buf.weight._value, np.float64).copy()

    noises, rec = [], []
    orig_randn = torch.randn
    orig_pre, orig_upd = TD3BC._preprocess_batch, TD3BC._update_with_batch

    def rec_randn(*a, **k):
        e = orig_randn(*a, **k)
        if "size" in k:
            noises.append(e.numpy().copy())
        return e

    def rec_pre(self, batch, buffer, indices):
        r = {"indices": np.array(indices, np.int64)}
        if prioritized:
            r["is_weight"] = np.array(batch.weight, np.float64)
        else:
            assert "weight" not in batch.get_keys()
        b = orig_pre(self, batch, buffer, indices)
        r["returns"] = b.returns.numpy().copy().reshape(-1)
        rec.append(r)
        return b

    def rec_upd(self, batch):
        stats = orig_upd(self, batch)
        rec[-1]["prio"] = batch.weight.detach().numpy().copy()
        rec[-1]["stats"] = np.array([stats.actor_loss, stats.critic1_loss, stats.critic2_loss])
        return stats

    torch.randn, TD3BC._preprocess_batch, TD3BC._update_with_batch = rec_randn, rec_pre, rec_upd
    try:
        np.random.seed(seed + 7)
        for u in range(n_updates):
            n0 = len(noises)
            with policy_within_training_step(algorithm.policy):
                algorithm.update(buffer=buf, sample_size=batch)
            assert len(noises) - n0 == 1
            out[f"u{u}_noise"] = noises[n0]
            for k, v in rec[-1].items():
                out[f"u{u}_{k}"] = v
            mods = [("actor", actor, AK), ("critic1", critic1, CK), ("critic2", critic2, CK),
                    ("actor_old", algorithm.actor_old.module, AK), ("critic1_old", algorithm.critic_old.module, CK),
                    ("critic2_old", algorithm.critic2_old.module, CK)]
            for name, mod, keys in mods:
                sd = mod.state_dict()
                out[f"u{u}_{name}"] = torch.cat([sd[k2].reshape(-1) for k2 in keys]).numpy()[::61].copy()
            if prioritized:
                out[f"u{u}_tree"] = np.asarray(buf.weight._value, np.float64).copy()
        for name, mod, keys, optim in (("actor", actor, AK, algorithm.policy_optim), ("critic1", critic1, CK, algorithm.critic_optim),
                                       ("critic2", critic2, CK, algorithm.critic2_optim)):
            params = dict(mod.named_parameters())
            st = [optim._optim.state[params[k]] for k in keys]
            out[f"adam_step_{name}"] = np.array(int(float(st[0]["step"])))
            out[f"adam_m_{name}"] = torch.cat([s["exp_avg"].reshape(-1) for s in st]).numpy()[::61].copy()
            out[f"adam_v_{name}"] = torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).numpy()[::61].copy()
    finally:
        torch.randn, TD3BC._preprocess_batch, TD3BC._update_with_batch = orig_randn, orig_pre, orig_upd
    cfg = dict(gamma=gamma, tau=tau, n_step=n_step, twin=1.0, policy_noise=policy_noise, noise_clip=noise_clip,
               update_actor_freq=update_actor_freq, max_action=max_action, actor_lr=actor_lr, critic_lr=critic_lr,
               alpha=algorithm.alpha, **({"tanh_trunks": 1.0} if activation is nn.Tanh else {}))
    out["cfg_keys"], out["cfg_vals"] = np.array(list(cfg.keys())), np.array(list(cfg.values()), np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"td3bc_{tag}.npz"), **out)


def main() -> None:
    gen_td3bc("offline", prioritized=False, E=4, slots=32, steps=30, obs_dim=23, act_dim=5, batch=64, n_updates=4, seed=51,
              hidden=((256, 256), (256, 256)), activation=nn.ReLU, max_action=1.0, alpha=2.5, update_actor_freq=2, n_step=1,
              actor_lr=3e-4, critic_lr=1e-3, tau=0.005, gamma=0.99)
    gen_td3bc("per_tanh", prioritized=True, E=4, slots=32, steps=30, obs_dim=17, act_dim=6, batch=48, n_updates=3, seed=52,
              hidden=((64, 48, 32), (40, 72, 56)), activation=nn.Tanh, max_action=1.5, alpha=1.0, update_actor_freq=1, n_step=3,
              actor_lr=3e-4, critic_lr=1e-3, tau=0.01, gamma=0.97)


if __name__ == "__main__":
    main()
