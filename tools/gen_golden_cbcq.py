"""TEST INFRASTRUCTURE ONLY - generates tests/golden/cbcq_d4rl.npz and tests/golden/cbcq_odd.npz by running the UNMODIFIED
reference on the CPU (where it is mounted; oracle/ref_shim.py makes it importable):

    python tools/gen_golden_cbcq.py

BCQ.update() (tianshou/algorithm/imitation/bcq.py) over a synthetic replay buffer:
  "d4rl":  the setup of examples/offline/d4rl_bcq.py -- perturbation net on a plain MLP[256, 256], critics Net[256, 256], VAE on
           MLP[512, 512], ReLU, L = 2 act_dim, phi 0.05, lmbda 0.75, R 10, max_action 1.  Perturbation.forward takes `[0]` of its
           preprocess net's output (continuous.py:409); a plain MLP returns a tensor, so that is the FIRST ROW of the logits and
           every row of the batch is perturbed by it -- the fixture records what the reference computes.
  "odd":   three nn.Tanh layers of 64 for the perturbation net (a `Net`, whose (logits, state) pair makes `[0]` the logits
           themselves: each row by its own) and the critics, VAE on MLP[96, 96], L 5, B 37, R 3, max_action 2, phi 0.3,
           lmbda 1, a critic2_optim of its own rate, max_grad_norm on both critics' optimizers.
Per update the file holds the sampled indices, the three normal draws in draw order (randn_like(std) [B, L], randn [B R, L],
randn [B, L]), the four statistics, the target, the critics' gradient norms where they are clipped and every 61st element of the
four networks and three lagged networks; once the buffer and every 61st element of the Adam moments at the end.  The initial
parameters are not stored: tests/oracle_cbcq.init_params rebuilds them from the seed (checked here against the reference
networks, tensor by tensor).  Only data is written; nothing of the reference's program text.
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
from torch import nn  # noqa: E402
import gymnasium as gym  # noqa: E402  (shim stub)

from tianshou.algorithm.imitation.bcq import BCQ, BCQPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import MLP, Net  # noqa: E402
from tianshou.utils.net.continuous import VAE, ContinuousCritic, Perturbation  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from tests import oracle_cbcq as OB  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
STRIDE = 61


def gen(tag: str, *, E: int, slots: int, steps: int, obs_dim: int, act_dim: int, latent_dim: int, batch: int, n_updates: int,
        seed: int, hidden, vae_hidden, activation, pert_net: str, phi: float, lmbda: float, R: int, max_action: float,
        pert_lr: float, critic_lr: float, critic2_lr: float | None, vae_lr: float, critic_max_grad_norm: float | None,
        tau: float = 0.005, gamma: float = 0.99) -> None:
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    hidden, vae_hidden = list(hidden), list(vae_hidden)
    if pert_net == "mlp":
        net_a = MLP(input_dim=obs_dim + act_dim, output_dim=act_dim, hidden_sizes=hidden, activation=activation)
    else:
        net_a = Net(state_shape=(obs_dim + act_dim,), action_shape=(act_dim,), hidden_sizes=hidden, activation=activation)
    actor = Perturbation(preprocess_net=net_a, max_action=max_action, phi=phi)
    mk_net = lambda: Net(state_shape=(obs_dim,), action_shape=(act_dim,), hidden_sizes=hidden, concat=True,  # noqa: E731
                         activation=activation)
    n1, n2 = mk_net(), mk_net()
    critic1, critic2 = ContinuousCritic(preprocess_net=n1), ContinuousCritic(preprocess_net=n2)
    enc = MLP(input_dim=obs_dim + act_dim, hidden_sizes=vae_hidden)
    dec = MLP(input_dim=obs_dim + latent_dim, output_dim=act_dim, hidden_sizes=vae_hidden)
    vae = VAE(encoder=enc, decoder=dec, hidden_dim=vae_hidden[-1], latent_dim=latent_dim, max_action=max_action)
    p0 = OB.init_params(obs_dim, act_dim, latent_dim, seed, hidden, vae_hidden)      # the tests rebuild the initial nets from the seed
    mods = {"pert": actor, "critic1": critic1, "critic2": critic2, "vae": vae}
    for pd, mod in zip(p0, mods.values()):
        sd = list(mod.state_dict().values())
        assert len(sd) == len(pd), (len(sd), len(pd))
        for a, (k, b) in zip(sd, pd.items()):
            assert torch.equal(a, b), f"oracle init differs from the reference at {k}"
    policy = BCQPolicy(actor_perturbation=actor, action_space=gym.spaces.Box(low=-max_action, high=max_action, shape=(act_dim,)),
                       critic=critic1, vae=vae)
    algorithm = BCQ(policy=policy, actor_perturbation_optim=AdamOptimizerFactory(lr=pert_lr),
                    critic_optim=AdamOptimizerFactory(lr=critic_lr), critic2=critic2,
                    critic2_optim=None if critic2_lr is None else AdamOptimizerFactory(lr=critic2_lr),
                    vae_optim=AdamOptimizerFactory(lr=vae_lr), gamma=gamma, tau=tau, lmbda=lmbda, num_sampled_action=R)
    if critic_max_grad_norm is not None:          # BCQ's constructor offers no argument for it; the wrapper's own attribute
        algorithm.critic_optim._max_grad_norm = critic_max_grad_norm
        algorithm.critic2_optim._max_grad_norm = critic_max_grad_norm
    lag = {"pert_old": algorithm.actor_perturbation_target, "critic1_old": algorithm.critic_target,
           "critic2_old": algorithm.critic2_target}
    buf = VectorReplayBuffer(E * slots, E)
    obs = rng.normal(size=(steps + 1, E, obs_dim)).astype(np.float32)
    act = rng.uniform(-max_action, max_action, size=(steps, E, act_dim)).astype(np.float32)
    rew = rng.normal(size=(steps, E)).astype(np.float32)
    term = rng.random((steps, E)) < 0.08
    trunc = (rng.random((steps, E)) < 0.04) & ~term
    for t in range(steps):
        buf.add(Batch(obs=obs[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=obs[t + 1]))
    out: dict[str, np.ndarray] = {"dims": np.array([E, slots, steps, obs_dim, act_dim, latent_dim, batch, n_updates, seed, R]),
                                  "hidden": np.array(hidden, np.int64), "vae_hidden": np.array(vae_hidden, np.int64)}
    for k2 in ("obs", "obs_next", "act"):
        out[k2] = np.asarray(getattr(buf, k2), np.float32)
    out["rew"], out["done"] = np.asarray(buf.rew, np.float64), np.asarray(buf.done, bool)

    draws: list[np.ndarray] = []
    norms: list[float] = []
    mses: list[tuple] = []
    orig_randn, orig_like, orig_mse, orig_clip = torch.randn, torch.randn_like, F.mse_loss, nn.utils.clip_grad_norm_

    def rec_randn(*a, **k):
        e = orig_randn(*a, **k)
        draws.append(e.numpy().copy())
        return e

    def rec_like(*a, **k):
        e = orig_like(*a, **k)
        draws.append(e.numpy().copy())
        return e

    def rec_mse(a, b, *r, **k):
        mses.append((a.detach().numpy().copy(), b.detach().numpy().copy()))
        return orig_mse(a, b, *r, **k)

    def rec_clip(parameters, max_norm, *a, **k):
        n = orig_clip(parameters, max_norm, *a, **k)
        norms.append(float(n))
        return n

    orig_sample = buf.sample_indices
    sampled: list[np.ndarray] = []

    def rec_sample(n):
        i = orig_sample(n)
        sampled.append(np.array(i, np.int64))
        return i

    buf.sample_indices = rec_sample
    torch.randn, torch.randn_like, F.mse_loss, nn.utils.clip_grad_norm_ = rec_randn, rec_like, rec_mse, rec_clip
    flat = lambda mod: torch.cat([v.reshape(-1) for v in mod.state_dict().values()]).numpy()[::STRIDE].copy()  # noqa: E731
    try:
        np.random.seed(seed + 7)
        for u in range(n_updates):
            d0, g0, m0 = len(draws), len(norms), len(mses)
            with policy_within_training_step(algorithm.policy):
                stats = algorithm.update(buffer=buf, sample_size=batch)
            d = draws[d0:]
            assert [x.shape for x in d] == [(batch, latent_dim), (batch * R, latent_dim), (batch, latent_dim)], [x.shape for x in d]
            out[f"u{u}_eps1"], out[f"u{u}_eps2"], out[f"u{u}_eps3"] = d
            m = mses[m0:]
            assert len(m) == 3 and m[0][0].shape == (batch, act_dim) and m[1][1].shape == (batch, 1)
            assert np.array_equal(m[1][1], m[2][1])
            out[f"u{u}_target"] = m[1][1].reshape(-1).copy()
            assert len(norms) - g0 == (0 if critic_max_grad_norm is None else 2)
            out[f"u{u}_grad_norms"] = np.array(norms[g0:], np.float64)
            out[f"u{u}_indices"] = sampled[-1]
            out[f"u{u}_stats"] = np.array([stats.actor_loss, stats.critic1_loss, stats.critic2_loss, stats.vae_loss], np.float64)
            for name, mod in {**mods, **lag}.items():
                out[f"u{u}_{name}"] = flat(mod)
        for name, mod, optim in (("pert", actor, algorithm.actor_perturbation_optim), ("critic1", critic1, algorithm.critic_optim),
                                 ("critic2", critic2, algorithm.critic2_optim), ("vae", vae, algorithm.vae_optim)):
            st = [optim._optim.state[p] for p in mod.parameters()]
            out[f"adam_step_{name}"] = np.array(int(float(st[0]["step"])))
            out[f"adam_m_{name}"] = torch.cat([s["exp_avg"].reshape(-1) for s in st]).numpy()[::STRIDE].copy()
            out[f"adam_v_{name}"] = torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).numpy()[::STRIDE].copy()
    finally:
        torch.randn, torch.randn_like, F.mse_loss, nn.utils.clip_grad_norm_ = orig_randn, orig_like, orig_mse, orig_clip
    assert any(np.asarray(buf.done)[i].any() for i in sampled), "no done row in any sampled batch"
    cfg = dict(gamma=gamma, tau=tau, lmbda=lmbda, phi=phi, max_action=max_action, num_sampled_action=float(R), pert_lr=pert_lr,
               critic1_lr=critic_lr, critic2_lr=critic_lr if critic2_lr is None else critic2_lr, vae_lr=vae_lr,
               critic1_max_grad_norm=critic_max_grad_norm or 0.0, critic2_max_grad_norm=critic_max_grad_norm or 0.0,
               pert_first_row=float(pert_net == "mlp"), tanh_trunks=float(activation is nn.Tanh))
    out["cfg_keys"], out["cfg_vals"] = np.array(list(cfg.keys())), np.array(list(cfg.values()), np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"cbcq_{tag}.npz"), **out)


def main() -> None:
    gen("d4rl", E=4, slots=32, steps=32, obs_dim=11, act_dim=3, latent_dim=6, batch=64, n_updates=3, seed=71, hidden=(256, 256),
        vae_hidden=(512, 512), activation=nn.ReLU, pert_net="mlp", phi=0.05, lmbda=0.75, R=10, max_action=1.0, pert_lr=1e-3,
        critic_lr=1e-3, critic2_lr=None, vae_lr=1e-3, critic_max_grad_norm=None)
    gen("odd", E=4, slots=32, steps=32, obs_dim=7, act_dim=4, latent_dim=5, batch=37, n_updates=3, seed=72, hidden=(64, 64, 64),
        vae_hidden=(96, 96), activation=nn.Tanh, pert_net="net", phi=0.3, lmbda=1.0, R=3, max_action=2.0, pert_lr=3e-4,
        critic_lr=1e-3, critic2_lr=5e-4, vae_lr=2e-3, critic_max_grad_norm=0.5, tau=0.01, gamma=0.97)


if __name__ == "__main__":
    main()
