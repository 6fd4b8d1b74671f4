"""TEST INFRASTRUCTURE ONLY - torch restatement of the discriminator half of the reference's GAIL update.

Never imported by the product (`tianshou_amd/`).  GAIL is PPO plus a discriminator: the PPO half is oracle/oracle_ppo.py's; what
is restated here is the reward, the discriminator loss, one discriminator step and the chunking rule.

Follows:
  reward      GAIL._preprocess_batch imitation/gail.py:203-206: rew = -logsigmoid(-D(obs, act))
  disc        gail.py:208-212: disc_net(cat([obs, act], dim=1)); Net / MLP (utils/net/common.py:90-178): Linear, activation per
              hidden layer, a linear head of one output
  loss        gail.py:229-235: -logsigmoid(-l_pi).mean() - logsigmoid(l_exp).mean(), (l_pi < 0).mean(), (l_exp > 0).mean()
  chunks      gail.py:224-225 + Batch.split(bsz, merge_last=True) data/batch.py:1199-1215: bsz = N // disc_update_num,
              N // bsz chunks, the last one takes the remainder; every step draws bsz expert rows (gail.py:227)
  step        Optimizer.step algorithm_base.py:484-500: clip_grad_norm_ then torch.optim.Adam's single-tensor arithmetic
The network is a list of nn.Linear-layout tensors [w1, b1, ..., w_head, b_head].  Everything follows the parameters' dtype and
device, so the same code in float64 is the reference of the kernel edge tests and on device tensors the eager baseline of the
benchmark.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

ACTIVATIONS = {"tanh": torch.tanh, "relu": torch.relu, "none": lambda x: x}


def init_disc(in_dim: int, hidden, seed: int, dtype=torch.float32, scale: float = 1.0) -> list[torch.Tensor]:
    """nn.Linear's default initialisation drawn from a seeded CPU generator (layer order), head of one output."""
    g = torch.Generator().manual_seed(seed)
    dims = [in_dim, *hidden, 1]
    t = []
    for i in range(len(dims) - 1):
        bound = 1.0 / dims[i] ** 0.5
        t.append(((torch.rand(dims[i + 1], dims[i], generator=g) * 2 - 1) * bound * scale).to(dtype))
        t.append(((torch.rand(dims[i + 1], generator=g) * 2 - 1) * bound * scale).to(dtype))
    return t


def disc_forward(t: list[torch.Tensor], obs: torch.Tensor, act: torch.Tensor, activation: str = "tanh") -> torch.Tensor:
    """gail.py:208-212 -> logits [B]."""
    f = ACTIVATIONS[activation]
    h = torch.cat([obs, act], dim=1).to(t[0].dtype)
    n = len(t) // 2
    for i in range(n):
        h = F.linear(h, t[2 * i], t[2 * i + 1])
        if i + 1 < n:
            h = f(h)
    return h.flatten()


def reward(t, obs, act, activation: str = "tanh") -> torch.Tensor:
    """gail.py:205."""
    with torch.no_grad():
        return -F.logsigmoid(-disc_forward(t, obs, act, activation))


def loss_terms(l_pi: torch.Tensor, l_exp: torch.Tensor):
    """gail.py:229-235 -> (loss with graph, acc_pi, acc_exp)."""
    loss = -F.logsigmoid(-l_pi).mean() + -F.logsigmoid(l_exp).mean()
    return loss, (l_pi < 0).to(l_pi.dtype).mean(), (l_exp > 0).to(l_exp.dtype).mean()


def loss_and_grad(logits: torch.Tensor, n_pi: int):
    """The loss kernel's contract on a vector of logits (policy rows first) -> (stats[3], d loss / d logits)."""
    l = logits.detach().clone().requires_grad_(True)
    loss, a_pi, a_exp = loss_terms(l[:n_pi], l[n_pi:])
    (g,) = torch.autograd.grad(loss, l)
    return torch.stack([loss.detach(), a_pi, a_exp]), g


def chunks(n: int, disc_update_num: int):
    """-> (bsz, [(start, stop) of every policy chunk of the split permutation]).  ValueError where the reference fails its
    assertion (bsz = 0)."""
    bsz = n // disc_update_num
    if bsz < 1:
        raise ValueError(f"len(batch) = {n} < disc_update_num = {disc_update_num}")
    steps = n // bsz
    return bsz, [(k * bsz, (k + 1) * bsz if k + 1 < steps else n) for k in range(steps)]


@dataclass
class Adam:
    lr: float = 1e-3
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    max_grad_norm: float | None = None
    m: list = field(default_factory=list)
    v: list = field(default_factory=list)
    step: int = 0

    def apply(self, params: list[torch.Tensor], grads: list[torch.Tensor]) -> list[torch.Tensor]:
        if self.max_grad_norm:                                   # nn.utils.clip_grad_norm_
            total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
            coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)
            grads = [g * coef for g in grads]
        if not self.m:
            self.m = [torch.zeros_like(g) for g in grads]
            self.v = [torch.zeros_like(g) for g in grads]
        self.step += 1
        b1, b2 = self.betas
        bc1, bc2 = 1 - b1 ** self.step, 1 - b2 ** self.step
        out = []
        for p, g, m, v in zip(params, grads, self.m, self.v):
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (v.sqrt() / bc2 ** 0.5).add_(self.eps)
            out.append(p.addcdiv(m, denom, value=-(self.lr / bc1)))
        return out


def disc_grad(t, obs_pi, act_pi, obs_exp, act_exp, activation: str = "tanh"):
    """One step's loss, accuracies and gradient (gail.py:226-231) -> (stats[3], [grads])."""
    p = [x.detach().clone().requires_grad_(True) for x in t]
    loss, a_pi, a_exp = loss_terms(disc_forward(p, obs_pi, act_pi, activation), disc_forward(p, obs_exp, act_exp, activation))
    gs = torch.autograd.grad(loss, p)
    return torch.stack([loss.detach(), a_pi, a_exp]), list(gs)


def disc_update(t, opt: Adam, obs, act, perm, obs_exp, act_exp, exp_index, disc_update_num: int, activation: str = "tanh"):
    """gail.py:220-235 with the draws as inputs: `perm` the split permutation of the N rollout rows, `exp_index` [steps, bsz]
    (or flat) the expert rows of every step -> (new tensors, stats [steps, 3])."""
    n = obs.shape[0]
    bsz, ch = chunks(n, disc_update_num)
    perm = torch.as_tensor(perm, dtype=torch.long, device=obs.device)
    ei = torch.as_tensor(exp_index, dtype=torch.long, device=obs.device).reshape(len(ch), bsz)
    stats = []
    for k, (a, b) in enumerate(ch):
        rows = perm[a:b]
        st, gs = disc_grad(t, obs[rows], act[rows], obs_exp[ei[k]], act_exp[ei[k]], activation)
        t = opt.apply(t, gs)
        stats.append(st)
    return t, torch.stack(stats)
