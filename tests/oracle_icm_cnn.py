"""TEST INFRASTRUCTURE ONLY - torch restatement of the reference's Intrinsic Curiosity Module on the Atari trunk and its update.

Never imported by the product (`tianshou_amd/`).  The model of examples/atari/atari_ppo.py:136-160:
  feature_net   DQNet(c, h, w, action_shape, features_only=True).net (atari_network.py): Conv2d(c, 32, 8, 4), ReLU,
                Conv2d(32, 64, 4, 2), ReLU, Conv2d(64, 64, 3, 1), ReLU, Flatten -- torch's (channel, h, w) feature order
  the rest      tests/oracle_icm.py: forward / inverse MLPs, mse, reward, loss and the optimizer step are shared with it
The model is three lists of torch-layout tensors: [conv1.w, conv1.b, conv2.w, conv2.b, conv3.w, conv3.b], forward [w1, b1, ...],
inverse [w1, b1, ...].  Frames come NHWC [B, h, w, c] (uint8 or float, raw values) as the engine takes them and are permuted to
NCHW here.  Everything follows the parameters' dtype and device: in float64 the reference of the kernel tests, on device tensors
in float32 the eager baseline of the benchmark.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.oracle_icm import Optim, loss_terms, mlp, reward  # noqa: F401  (re-exported: the CNN tests use them through this module)

CONVS = ((32, 8, 4), (64, 4, 2), (64, 3, 1))


def feature_dim(h: int, w: int) -> int:
    for _, k, s in CONVS:
        h, w = (h - k) // s + 1, (w - k) // s + 1
    return 64 * h * w


def init_model(c: int, h: int, w: int, n_act: int, model_hidden, seed: int, dtype=torch.float32):
    """-> [conv, forward, inverse] from `np.random.RandomState(seed)` (a frozen stream), uniform in +-fan_in^-1/2 per layer."""
    rs = np.random.RandomState(seed)
    f = feature_dim(h, w)

    def layer(shape, fan_in):
        b = fan_in ** -0.5
        return [torch.from_numpy(rs.uniform(-b, b, size=shape)).to(dtype), torch.from_numpy(rs.uniform(-b, b, size=shape[0])).to(dtype)]

    conv, ic = [], c
    for oc, k, _ in CONVS:
        conv += layer((oc, ic, k, k), ic * k * k)
        ic = oc
    chains = []
    for dims in ([f + n_act, *model_hidden, f], [2 * f, *model_hidden, n_act]):
        t = []
        for kk, n in zip(dims[:-1], dims[1:]):
            t += layer((n, kk), kk)
        chains.append(t)
    return [conv, *chains]


def features(conv, obs_nhwc, pre: list | None = None):
    """phi [B, F] in torch's flatten order; `pre` collects the three pre-activations."""
    x = obs_nhwc.to(conv[0].dtype).permute(0, 3, 1, 2)
    for i, (_, _, s) in enumerate(CONVS):
        z = F.conv2d(x, conv[2 * i], conv[2 * i + 1], stride=s)
        if pre is not None:
            pre.append(z)
        x = torch.relu(z)
    return x.flatten(1)


def parts(model, obs, act, obs_next):
    conv, fwd, inv = model
    dt = conv[0].dtype
    n_act = inv[-1].numel()
    phi1, phi2 = features(conv, obs), features(conv, obs_next)
    phi2_hat = mlp(fwd, torch.cat([phi1, F.one_hot(act.long(), n_act).to(dt)], dim=1))
    return phi2_hat, phi2, mlp(inv, torch.cat([phi1, phi2], dim=1))


def forward(model, obs, act, obs_next):
    """discrete.py:410-428 -> (mse_loss [B], act_hat [B, A]) with graph."""
    phi2_hat, phi2, act_hat = parts(model, obs, act, obs_next)
    return 0.5 * ((phi2_hat - phi2) ** 2).sum(1), act_hat


def grads(model, obs, act, obs_next, w: float, lr_scale: float):
    """-> (stats[3], [conv grads, forward grads, inverse grads], mse, act_hat) at `model`."""
    leaves = [[x.detach().clone().requires_grad_(True) for x in chain] for chain in model]
    mse, act_hat = forward(leaves, obs, act, obs_next)
    loss, fl, il = loss_terms(mse, act_hat, act, w, lr_scale)
    flat = [x for chain in leaves for x in chain]
    gs = torch.autograd.grad(loss, flat, allow_unused=True)
    gs = [torch.zeros_like(x) if g is None else g for g, x in zip(gs, flat)]
    out, o = [], 0
    for chain in leaves:
        out.append(gs[o:o + len(chain)])
        o += len(chain)
    return torch.stack([loss.detach(), fl.detach(), il.detach()]), out, mse.detach(), act_hat.detach()


def update(optim: Optim, obs, act, obs_next, w: float, lr_scale: float):
    """icm.py:90-109: one step on the whole batch -> stats[3] at the parameters before the step."""
    stats, gs, _, _ = grads(optim.model(), obs, act, obs_next, w, lr_scale)
    optim.step(gs)
    return stats


def cast(model, dtype=None, device=None):
    return [[x.to(dtype=dtype, device=device) for x in chain] for chain in model]


def flat_tensors(model) -> list[torch.Tensor]:
    """The tensor list `tianshou_amd.icm_cnn.flat_from_torch` takes."""
    return [x for chain in model for x in chain]


PPO_SHAPES = lambda c, f, n_act: [(32, c, 8, 8), (64, 32, 4, 4), (64, 64, 3, 3), (512, f), (n_act, 512), (1, 512)]  # noqa: E731


def init_ppo(c: int, h: int, w: int, n_act: int, seed: int, dtype=torch.float32) -> list[torch.Tensor]:
    """The twelve tensors of the atari_ppo.py actor-critic in HipPPOCnn's order (conv1..3, fc, actor head, critic head), from
    `np.random.RandomState(seed)`, uniform in +-fan_in^-1/2 per layer."""
    rs, out = np.random.RandomState(seed), []
    for shape in PPO_SHAPES(c, feature_dim(h, w), n_act):
        b = float(np.prod(shape[1:])) ** -0.5
        out += [torch.from_numpy(rs.uniform(-b, b, size=shape)).to(dtype), torch.from_numpy(rs.uniform(-b, b, size=shape[0])).to(dtype)]
    return out


def relu_margins(model, obs, act, obs_next):
    """Per ReLU layer of the model (conv1..3 on [obs; obs_next], the hidden layers of the forward and the inverse model):
    (min |z| in float64, the largest |z32 - z64|) -> two float64 arrays.  `model` in float32; frames NHWC."""
    def pre(m):
        z = []
        x = torch.cat([obs, obs_next])
        phi = features(m[0], x, z)
        b = obs.shape[0]
        n_act = m[2][-1].numel()
        xs = (torch.cat([phi[:b], F.one_hot(act.long(), n_act).to(phi.dtype)], 1), torch.cat([phi[:b], phi[b:]], 1))
        for t, xin in zip(m[1:], xs):
            for i in range(len(t) // 2 - 1):
                zz = F.linear(xin, t[2 * i], t[2 * i + 1])
                z.append(zz)
                xin = torch.relu(zz)
        return z

    with torch.no_grad():
        z32, z64 = pre(cast(model, torch.float32)), pre(cast(model, torch.float64))
    return (np.array([float(b.abs().min()) for b in z64]), np.array([float((a.double() - b).abs().max()) for a, b in zip(z32, z64)]))
