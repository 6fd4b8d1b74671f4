"""TEST INFRASTRUCTURE ONLY - generates tests/golden/icm_cnn_small.npz and tests/golden/icm_cnn_odd.npz by running the UNMODIFIED
reference (where it is mounted; oracle/ref_shim.py makes it importable) on the CPU:

    python tools/gen_golden_icm_cnn.py [small|odd] [first_seed] [seeds]

ICMOnPolicyWrapper.update() (tianshou/algorithm/modelbased/icm.py) twice in a row around PPO with the networks of
examples/atari/atari_ppo.py:106-171 -- DQNet(features_only=True, output_dim_added_layer=512) shared by DiscreteActor(logits) and
DiscreteCritic; IntrinsicCuriosityModule(feature_net=DQNet(features_only=True).net, feature_dim=64 OH3 OW3) -- on a synthetic
VectorReplayBuffer of uint8 frames:
"small" -- c = 4, 36 x 36 (F = 64), 6 actions, hidden_sizes [64], 2 envs x 24 steps of whole [c, h, w] frames, obs_next stored,
minibatch 16, repeat 2; "odd" -- 44 x 36 (F = 128), 3 actions, hidden_sizes (), stack_num = 4 with save_only_last_obs and
ignore_obs_next, one episode end and one truncation inside, recompute_advantage, return_scaling, reward_scale 0.5,
forward_loss_weight 0.9, lr_scale 0.3.
The frames are Atari-like: a zero background with a few small sprites of raw 0..255 values that move now and then (`sprites`).
Per update the file holds what icm_*.npz holds (rewards before and after, mse_loss, strided act_hat, v_s / returns / advantages /
logp_old, the three ICM statistics, the PPO losses and permutations, strided parameters), strided optimizer moments at the end.
The INITIAL parameters of both networks are not stored: tests/oracle_icm_cnn.py rebuilds them from the stored seed
(np.random.RandomState, uniform in +-fan_in^-1/2 per layer; that legacy stream is frozen) -- the files stay below 1 MB.
ReLU margin: raw frames make pre-activations of order 10^2, so an absolute margin means nothing here.  Per ReLU layer of the ICM
model (conv1..3 over [obs; obs_next], the models' hidden layers) the pre-activations are evaluated in float32 and in float64; a
seed is taken only if min |z| >= 64 x the largest float32-vs-float64 difference seen at that layer, in both updates (asserted);
both numbers are stored (`relu_min_abs`, `relu_f32_err`, [updates, layers]).  Only data is written; nothing of the reference's
program text.
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

from tianshou.algorithm.modelbased.icm import ICMOnPolicyWrapper  # noqa: E402
from tianshou.algorithm.modelfree.ppo import PPO  # noqa: E402
from tianshou.algorithm.modelfree.reinforce import DiscreteActorPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, SequenceSummaryStats, VectorReplayBuffer  # noqa: E402
from tianshou.env.atari.atari_network import DQNet  # noqa: E402
from tianshou.utils.net.discrete import DiscreteActor, DiscreteCritic, IntrinsicCuriosityModule  # noqa: E402
from tianshou.utils.torch_utils import policy_within_training_step  # noqa: E402

from tests import oracle_icm_cnn as OC  # noqa: E402

OUT = os.environ.get("TS_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
STRIDE = 13
MARGIN = 64.0
TRUNK = ["preprocess.net.0.0.weight", "preprocess.net.0.0.bias", "preprocess.net.0.2.weight", "preprocess.net.0.2.bias",
         "preprocess.net.0.4.weight", "preprocess.net.0.4.bias", "preprocess.net.1.weight", "preprocess.net.1.bias"]
HEAD = ["last.model.0.weight", "last.model.0.bias"]


def strided(ts) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1) for t in ts]).numpy()[::STRIDE].copy()


def sprites(rng, T: int, E: int, planes: int, h: int, w: int, n: int = 2, cell: int = 4, p_move: float = 0.1) -> np.ndarray:
    """uint8 [T + 1, E, planes, h, w]: zero background, per plane `n` sprites of cell x cell raw 0..255 pixels that sit on a
    grid of `cell` pixels (conv1's stride) and move one cell with probability `p_move` per step.  Most consecutive frames are
    equal and windows repeat, as on a real Atari screen: the rollout holds a few thousand DISTINCT pre-activations per layer
    instead of a few hundred thousand, which is what lets a seed meet the ReLU margin at all."""
    f = np.zeros((T + 1, E, planes, h, w), np.uint8)
    hi = np.array([h // cell - 1, w // cell - 1])
    pos = rng.integers(0, hi + 1, size=(E, planes, n, 2))
    pix = rng.integers(1, 256, size=(E, planes, n, cell, cell), dtype=np.uint8)
    for t in range(T + 1):
        for e in range(E):
            for p in range(planes):
                for k in range(n):
                    y, x = pos[e, p, k] * cell
                    f[t, e, p, y:y + cell, x:x + cell] = pix[e, p, k]
        step = rng.integers(-1, 2, size=pos.shape) * (rng.random(pos.shape[:3]) < p_move)[..., None]
        pos = np.clip(pos + step, 0, hi)
    return f


def icm_model(icm) -> list:
    """The reference module's tensors as tests/oracle_icm_cnn.py's model."""
    lin = lambda mod: [p for m in mod.modules() if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]  # noqa: E731
    conv = [p for m in icm.feature_net.modules() if isinstance(m, torch.nn.Conv2d) for p in (m.weight, m.bias)]
    return [conv, lin(icm.forward_model), lin(icm.inverse_model)]


def run(tag: str, seed: int, *, E: int, T: int, c: int, h: int, w: int, n_act: int, model_hidden, batch_size: int, repeat: int,
        lr: float, icm_lr: float, lr_scale: float, reward_scale: float, forward_loss_weight: float, stacked: bool, n_updates: int = 2,
        **ppo_kwargs):
    """-> (dict to save or None when a margin fails, [updates, layers] min |z|, the same of the float32 error)."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    N = E * T
    net = DQNet(c=c, h=h, w=w, action_shape=n_act, features_only=True, output_dim_added_layer=512)
    actor, critic = DiscreteActor(preprocess_net=net, action_shape=n_act, softmax_output=False), DiscreteCritic(preprocess_net=net)
    ppo_par = [dict(actor.named_parameters())[k] for k in TRUNK + HEAD] + [dict(critic.named_parameters())[k] for k in HEAD]
    feature_net = DQNet(c=c, h=h, w=w, action_shape=n_act, features_only=True)
    f_dim = int(feature_net.output_dim)
    assert f_dim == OC.feature_dim(h, w)
    icm = IntrinsicCuriosityModule(feature_net=feature_net.net, feature_dim=f_dim, action_dim=n_act, hidden_sizes=list(model_hidden))
    icm_par = [p for chain in icm_model(icm) for p in chain]
    with torch.no_grad():                                   # the initial parameters: rebuilt in the tests from `seed`
        for p, t in zip(ppo_par, OC.init_ppo(c, h, w, n_act, seed)):
            p.copy_(t)
        for p, t in zip(icm_par, OC.flat_tensors(OC.init_model(c, h, w, n_act, list(model_hidden), seed + 1))):
            p.copy_(t)
    policy = DiscreteActorPolicy(actor=actor, action_space=gym.spaces.Discrete(n_act))
    ppo = PPO(policy=policy, critic=critic, optim=AdamOptimizerFactory(lr=lr), **ppo_kwargs)
    algorithm = ICMOnPolicyWrapper(wrapped_algorithm=ppo, model=icm, optim=AdamOptimizerFactory(lr=icm_lr), lr_scale=lr_scale,
                                   reward_scale=reward_scale, forward_loss_weight=forward_loss_weight)
    out: dict[str, np.ndarray] = {
        "dims": np.array([E, T, c, h, w, n_act, batch_size, repeat, seed, n_updates, STRIDE, int(stacked), f_dim]),
        "model_hidden": np.array(model_hidden, np.int64)}

    perms, seqs, pre = [], [], {}
    orig_perm, orig_from, orig_pre = np.random.permutation, SequenceSummaryStats.from_sequence.__func__, ICMOnPolicyWrapper._preprocess_batch
    zmin, zerr = [], []

    class Rejected(Exception):
        pass

    def rec_perm(n):
        q = orig_perm(n)
        perms.append(np.asarray(q, np.int64))
        return q

    def rec_from(c_, seq):
        seqs.append(np.asarray(seq, np.float64))
        return orig_from(c_, seq)

    def rec_pre(self, batch, buffer, indices):
        rew0 = np.asarray(buffer.rew[indices], np.float64).copy()
        nhwc = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint8))).permute(0, 2, 3, 1)  # noqa: E731
        model = [[t.detach().clone() for t in ch] for ch in icm_model(icm)]
        lo, err = OC.relu_margins(model, nhwc(batch.obs), torch.as_tensor(np.asarray(batch.act)), nhwc(batch.obs_next))
        zmin.append(lo)
        zerr.append(err)
        if not bool((lo >= MARGIN * err).all()):
            raise Rejected
        b = orig_pre(self, batch, buffer, indices)
        assert b.rew.dtype == np.float64
        pre.update(rew_before=rew0, rew_after=np.asarray(b.rew, np.float64).copy(), mse=b.policy.mse_loss.detach().numpy().copy(),
                   act_hat=b.policy.act_hat.detach().numpy().reshape(-1)[::STRIDE].copy(), v_s=b.v_s.numpy().copy(),
                   returns=b.returns.numpy().copy(), adv=b.adv.numpy().copy(), logp_old=b.logp_old.numpy().copy(),
                   indices=np.asarray(indices, np.int64), next_indices=np.asarray(buffer.next(indices), np.int64))
        return b

    np.random.permutation, SequenceSummaryStats.from_sequence = rec_perm, classmethod(rec_from)
    ICMOnPolicyWrapper._preprocess_batch = rec_pre
    try:
        act = rng.integers(0, n_act, size=(T, E))
        rew = rng.normal(size=(T, E)).astype(np.float32)
        term = rng.random((T, E)) < 0.06
        trunc = (rng.random((T, E)) < 0.05) & ~term
        if stacked:                                          # one episode end and one truncation inside, whatever the draw
            term[T // 3, 0], trunc[T // 3, 0] = True, False
            trunc[T // 2, E - 1], term[T // 2, E - 1] = True, False
            buf = VectorReplayBuffer(N, E, stack_num=c, save_only_last_obs=True, ignore_obs_next=True)
            fr = sprites(rng, T, E, 1, h, w, p_move=0.05)[:, :, 0]                        # [T + 1, E, h, w]: one new frame per step
            for t in range(T):
                st = np.repeat(fr[t][:, None], c, axis=1)                         # (only the last plane is stored)
                buf.add(Batch(obs=st, act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t],
                              obs_next=np.repeat(fr[t + 1][:, None], c, axis=1)))
        else:
            buf = VectorReplayBuffer(N, E)
            fr = sprites(rng, T, E, c, h, w)
            for t in range(T):
                buf.add(Batch(obs=fr[t], act=act[t], rew=rew[t], terminated=term[t], truncated=trunc[t], obs_next=fr[t + 1]))
            out["obs_next"] = np.asarray(buf.obs_next, np.uint8)
        out["obs"], out["act"] = np.asarray(buf.obs, np.uint8), np.asarray(buf.act, np.int64)
        out["rew"] = np.asarray(buf.rew, np.float64)
        out["terminated"], out["truncated"] = np.asarray(buf.terminated, bool), np.asarray(buf.truncated, bool)
        np.random.seed(seed + 100)
        for u in range(n_updates):
            p0, s0 = len(perms), len(seqs)
            with policy_within_training_step(algorithm.policy):
                stats = algorithm.update(buffer=buf, batch_size=batch_size, repeat=repeat)
            assert len(perms) - p0 == repeat and len(seqs) - s0 == 4
            out[f"u{u}_perms"] = np.stack(perms[p0:])
            out[f"u{u}_losses"] = np.stack(seqs[s0:s0 + 4], axis=1)       # loss, clip loss, vf loss, entropy loss (ppo.py:218-222)
            out[f"u{u}_icm_stats"] = np.array([stats.icm_loss, stats.icm_forward_loss, stats.icm_inverse_loss], np.float64)
            out[f"u{u}_gradient_steps"] = np.array(stats.gradient_steps)
            for k, v in pre.items():
                out[f"u{u}_pre_{k}"] = v
            out[f"u{u}_p"], out[f"u{u}_i"] = strided(ppo_par), strided(icm_par)
    except Rejected:
        return None, np.array(zmin), np.array(zerr)
    finally:
        np.random.permutation, SequenceSummaryStats.from_sequence = orig_perm, classmethod(orig_from)
        ICMOnPolicyWrapper._preprocess_batch = orig_pre
    for name, opt, par in (("p", ppo.optim._optim, ppo_par), ("i", algorithm.optim._optim, icm_par)):
        out[f"adam_step_{name}"] = np.array(int(float(opt.state[par[0]]["step"])))
        out[f"adam_m_{name}"] = strided([opt.state[p]["exp_avg"] for p in par])
        out[f"adam_v_{name}"] = strided([opt.state[p]["exp_avg_sq"] for p in par])
    out["ret_rms"] = np.array([ppo.ret_rms.mean, ppo.ret_rms.var, ppo.ret_rms.count], np.float64)
    cfg = dict(gamma=ppo.gamma, gae_lambda=ppo.gae_lambda, eps_clip=ppo.eps_clip, dual_clip=ppo.dual_clip or 0.0,
               value_clip=float(ppo.value_clip), advantage_normalization=float(ppo.advantage_normalization),
               recompute_advantage=float(ppo.recompute_adv), vf_coef=ppo.vf_coef, ent_coef=ppo.ent_coef,
               max_grad_norm=ppo.optim._max_grad_norm or 0.0, return_scaling=float(ppo.return_scaling), lr=lr, icm_lr=icm_lr,
               lr_scale=lr_scale, reward_scale=reward_scale, forward_loss_weight=forward_loss_weight)
    out["cfg_keys"], out["cfg_vals"] = np.array(list(cfg.keys())), np.array(list(cfg.values()), np.float64)
    out["relu_min_abs"], out["relu_f32_err"] = np.array(zmin), np.array(zerr)
    return out, np.array(zmin), np.array(zerr)


CONFIGS = {
    "small": dict(E=2, T=24, c=4, h=36, w=36, n_act=6, model_hidden=[64], batch_size=16, repeat=2, lr=2.5e-4, icm_lr=2.5e-4,
                  lr_scale=1.0, reward_scale=0.01, forward_loss_weight=0.2, stacked=False, eps_clip=0.1, vf_coef=0.25, ent_coef=0.01,
                  max_grad_norm=0.5, value_clip=True, dual_clip=None, advantage_normalization=True, recompute_advantage=False,
                  return_scaling=False, gae_lambda=0.95, gamma=0.99),
    "odd": dict(E=2, T=19, c=4, h=44, w=36, n_act=3, model_hidden=[], batch_size=16, repeat=2, lr=1e-3, icm_lr=2e-3, lr_scale=0.3,
                reward_scale=0.5, forward_loss_weight=0.9, stacked=True, eps_clip=0.2, vf_coef=0.25, ent_coef=0.01, max_grad_norm=0.5,
                value_clip=True, dual_clip=None, advantage_normalization=True, recompute_advantage=True, return_scaling=True,
                gae_lambda=0.9, gamma=0.98),
}


def gen(tag: str, first: int = 0, seeds: int = 4000) -> None:
    for seed in range(first, first + seeds):
        out, lo, err = run(tag, seed, **CONFIGS[tag])
        worst = float((lo / np.maximum(err, 1e-300)).min())
        print(f"icm_cnn_{tag}: seed {seed}: updates checked {len(lo)}, smallest min |z| / float32 error = {worst:.1f}", flush=True)
        if out is not None:
            break
    assert out is not None, f"icm_cnn_{tag}: no seed keeps every ReLU pre-activation {MARGIN} float32 errors away from zero"
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"icm_cnn_{tag}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    tags = [sys.argv[1]] if len(sys.argv) > 1 else list(CONFIGS)
    for t in tags:
        gen(t, *(int(x) for x in sys.argv[2:4]))
