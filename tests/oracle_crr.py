"""TEST INFRASTRUCTURE ONLY - torch autograd restatement of the reference's DiscreteCRR path on the Atari trunk.

Never imported by the product (`tianshou_amd/`).  Lives under tests/ next to the tests that use it; the buffer arithmetic
comes from oracle/oracle.py and oracle/oracle_dqn.py.

Follows:
  net       DiscreteActor(preprocess_net, hidden_sizes=[512], softmax_output=False) and DiscreteCritic(preprocess_net,
            hidden_sizes=[512], last_size=n_act) on ONE DQNet(features_only=True) trunk (examples/offline/atari_crr.py)
  target    discrete_crr.py:135-142: rew + gamma * (done > 0 ? 0 : sum_j softmax(l_old)_j q_old_j) on obs_next, the lagged
            pair (the live pair with target_update_freq == 0), no gradient
  update    discrete_crr.py:125-167: lagged refresh at iter % freq == 0, critic + advantage-weighted actor + CQL loss with
            the weight NOT detached, clip_grad_norm_ and ONE torch.optim.Adam over the 14 tensors.  Both [B] against [B, 1]
            broadcasts are kept as the reference writes them: the actor loss is the mean of the [B, B] product of
            -log_prob(act) and the weight, i.e. mean(nll) * mean(coef), and the CQL mean runs over B x B terms too
Gradients come from autograd, never from the closed forms (`closed_form_grads` states those, for the tests that compare).
Tensors follow the parameters' device and dtype, so the same code is the float64 yardstick of the tolerances and the eager
baseline of bench_crr.py on a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from oracle import oracle_dqn as OD

# ModuleList([policy, critic]).named_parameters(): the shared trunk once (under the actor), the actor head, the critic head
PARAM_ORDER = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b",
               "a1.w", "a1.b", "a2.w", "a2.b", "c1.w", "c1.b", "c2.w", "c2.b"]
TIANSHOU_KEYS = ["0.actor.preprocess.net.0.weight", "0.actor.preprocess.net.0.bias", "0.actor.preprocess.net.2.weight",
                 "0.actor.preprocess.net.2.bias", "0.actor.preprocess.net.4.weight", "0.actor.preprocess.net.4.bias",
                 "0.actor.last.model.0.weight", "0.actor.last.model.0.bias", "0.actor.last.model.2.weight",
                 "0.actor.last.model.2.bias", "1.last.model.0.weight", "1.last.model.0.bias", "1.last.model.2.weight",
                 "1.last.model.2.bias"]
HIDDEN = 512
MODES = ("exp", "binary", "all")


@dataclass
class CRRConfig:
    gamma: float = 0.99
    policy_improvement_mode: str = "exp"
    ratio_upper_bound: float = 20.0
    beta: float = 1.0
    min_q_weight: float = 10.0
    target_update_freq: int = 0
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    max_grad_norm: float | None = None


def feature_dim(h: int, w: int) -> int:
    oh, ow = OD.conv_out_hw(h, w)[-1]
    return 64 * oh * ow


def init_params(c: int, h: int, w: int, n_act: int, seed: int = 0) -> dict[str, torch.Tensor]:
    """Same RNG consumption as `torch.manual_seed(seed)` + the example's construction: the DQNet trunk, the actor's MLP, the
    critic's MLP (tools/gen_golden_crr.py asserts the equality tensor by tensor)."""
    torch.manual_seed(seed)
    f = feature_dim(h, w)
    mods = {"conv1": torch.nn.Conv2d(c, 32, 8, 4), "conv2": torch.nn.Conv2d(32, 64, 4, 2), "conv3": torch.nn.Conv2d(64, 64, 3, 1),
            "a1": torch.nn.Linear(f, HIDDEN), "a2": torch.nn.Linear(HIDDEN, n_act),
            "c1": torch.nn.Linear(f, HIDDEN), "c2": torch.nn.Linear(HIDDEN, n_act)}
    p = {}
    for name, m in mods.items():
        p[name + ".w"] = m.weight.detach().clone()
        p[name + ".b"] = m.bias.detach().clone()
    return p


def features(p, obs) -> torch.Tensor:
    ref = p["conv1.w"]
    x = torch.as_tensor(np.asarray(obs) if not isinstance(obs, torch.Tensor) else obs).to(ref.device, ref.dtype)
    x = F.relu(F.conv2d(x, p["conv1.w"], p["conv1.b"], stride=4))
    x = F.relu(F.conv2d(x, p["conv2.w"], p["conv2.b"], stride=2))
    x = F.relu(F.conv2d(x, p["conv3.w"], p["conv3.b"], stride=1))
    return x.flatten(1)


def head(p, feat, which: str) -> torch.Tensor:
    return F.linear(F.relu(F.linear(feat, p[which + "1.w"], p[which + "1.b"])), p[which + "2.w"], p[which + "2.b"])


def heads(p, obs):
    """-> (q [B, A] of the critic, logits [B, A] of the actor)."""
    feat = features(p, obs)
    return head(p, feat, "c"), head(p, feat, "a")


def _on(x, like: torch.Tensor, dtype=None) -> torch.Tensor:
    """A host array or a tensor on any device -> a tensor on `like`'s device."""
    x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return x.to(device=like.device, dtype=dtype if dtype is not None else like.dtype)


def expected_target(q_old, l_old, rew, done, gamma: float) -> torch.Tensor:
    """discrete_crr.py:137-142 on head outputs -> [B]."""
    with torch.no_grad():
        ev = (q_old * Categorical(logits=l_old).probs).sum(-1, keepdim=True)
        ev[_on(done, q_old, torch.int64) > 0] = 0.0
        rew = _on(rew, q_old)
        return (rew.unsqueeze(1) + gamma * ev).flatten()


def losses_from_heads(q, lg, act, target, mode: str, beta: float, ratio_upper_bound: float, min_q_weight: float,
                      per_sample: bool = False):
    """discrete_crr.py:131-158 on head outputs -> (loss, actor_loss, critic_loss, cql_loss: scalar tensors with graph, adv [B]).
    per_sample: the forms the kernels compute -- mean(nll) * mean(coef) and mean_b (lse_b - qa_b) -- instead of the
    reference's two [B] against [B, 1] broadcast means over B x B terms."""
    act = _on(act, q, torch.int64).flatten()
    target = _on(target, q).reshape(-1, 1)
    qa = q.gather(1, act.unsqueeze(1))
    critic_loss = 0.5 * F.mse_loss(qa, target)
    dist = Categorical(logits=lg)
    adv = qa - (q * dist.probs).sum(-1, keepdim=True)
    if mode == "binary":
        coef = (adv > 0).to(q.dtype)
    elif mode == "exp":
        coef = (adv / beta).exp().clamp(0, ratio_upper_bound)
    else:
        assert mode == "all", mode
        coef = 1.0
    if per_sample:
        cbar = coef.mean() if isinstance(coef, torch.Tensor) else coef
        actor_loss = (-dist.log_prob(act)).mean() * cbar
        cql_loss = (q.logsumexp(1) - qa.flatten()).mean()
    else:
        actor_loss = (-dist.log_prob(act) * coef).mean()              # [B] * [B, 1]: the mean of a [B, B] product
        cql_loss = (q.logsumexp(1) - qa).mean()                       # [B] - [B, 1]: B x B terms again
    loss = actor_loss + critic_loss + min_q_weight * cql_loss
    return loss, actor_loss, critic_loss, cql_loss, adv.flatten()


def closed_form_grads(q, lg, act, target, mode: str, beta: float, ratio_upper_bound: float, min_q_weight: float):
    """The head gradients as the gradient kernel writes them -> (dq [B, A], dl [B, A])."""
    q, lg = q.detach(), lg.detach()
    b, a = q.shape
    act = _on(act, q, torch.int64).flatten()
    y = _on(target, q).flatten()
    hot = F.one_hot(act, a).to(q)
    pi = torch.softmax(lg, 1)
    nll = (torch.logsumexp(lg, 1) - lg.gather(1, act[:, None]).flatten())
    qa = q.gather(1, act[:, None]).flatten()
    v = (pi * q).sum(1)
    adv = qa - v
    g = torch.zeros_like(adv)
    if mode == "exp":
        e = (adv / beta).exp()
        coef = e.clamp(0, ratio_upper_bound)
        g = torch.where(e <= ratio_upper_bound, nll.mean(), torch.zeros_like(e)) * e / beta
    elif mode == "binary":
        coef = (adv > 0).to(q)
    else:
        coef = torch.ones_like(adv)
    dq = ((qa - y)[:, None] * hot + min_q_weight * (torch.softmax(q, 1) - hot)) / b
    dl = coef.mean() * (pi - hot) / b
    if mode == "exp":
        dq = dq + g[:, None] * (hot - pi) / b
        dl = dl - g[:, None] * pi * (q - v[:, None]) / b
    return dq, dl


class CRRState:
    """Live parameters (leaf tensors under ONE torch.optim.Adam), the lagged copy (None with target_update_freq == 0), `iter`."""

    def __init__(self, p: dict[str, torch.Tensor], cfg: CRRConfig):
        self.params = {k: p[k].detach().clone().requires_grad_(True) for k in PARAM_ORDER}
        self.opt = torch.optim.Adam([self.params[k] for k in PARAM_ORDER], lr=cfg.lr, betas=cfg.betas, eps=cfg.adam_eps)
        self.params_old = {k: p[k].detach().clone() for k in PARAM_ORDER} if cfg.target_update_freq > 0 else None
        self.iter = 0

    @property
    def adam_step(self) -> int:
        st = self.opt.state.get(self.params[PARAM_ORDER[0]])
        return int(float(st["step"])) if st else 0

    def moments(self, which: str) -> dict[str, torch.Tensor]:
        """which: "exp_avg" | "exp_avg_sq" -> per-tensor moments (zeros before the first step)."""
        return {k: (self.opt.state[v][which] if self.opt.state.get(v) else torch.zeros_like(v)) for k, v in self.params.items()}


def make_state(p, cfg: CRRConfig) -> CRRState:
    return CRRState(p, cfg)


def update_with_batch(st: CRRState, cfg: CRRConfig, obs, obs_next, act, rew, done, collect: dict | None = None,
                      apply: bool = True):
    """discrete_crr.py:125-167 -> (loss, actor_loss, critic_loss, cql_loss) floats.  apply=False: the gradient only (in
    collect["grads"]); nothing is synced, stepped or counted."""
    if apply and cfg.target_update_freq > 0 and st.iter % cfg.target_update_freq == 0:
        st.params_old = {k: v.detach().clone() for k, v in st.params.items()}
    p = st.params
    for v in p.values():
        v.grad = None
    q, lg = heads(p, obs)
    with torch.no_grad():
        old = st.params_old if cfg.target_update_freq > 0 else {k: v.detach() for k, v in p.items()}
        q_old, l_old = heads(old, obs_next)
    target = expected_target(q_old, l_old, rew, done, cfg.gamma)
    loss, actor_loss, critic_loss, cql_loss, adv = losses_from_heads(
        q, lg, act, target, cfg.policy_improvement_mode, cfg.beta, cfg.ratio_upper_bound, cfg.min_q_weight)
    loss.backward()
    if collect is not None:
        collect["q"], collect["logits"], collect["adv"] = q.detach().clone(), lg.detach().clone(), adv.detach().clone()
        collect["target"] = target.clone()
        collect["grads"] = {k: v.grad.clone() for k, v in p.items()}
    if apply:
        if cfg.max_grad_norm:
            torch.nn.utils.clip_grad_norm_(list(p.values()), cfg.max_grad_norm)
        for g in st.opt.param_groups:
            g["lr"] = cfg.lr
        st.opt.step()
        st.iter += 1
    return tuple(float(x.item()) for x in (loss, actor_loss, critic_loss, cql_loss))
