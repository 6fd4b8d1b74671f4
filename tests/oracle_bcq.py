"""TEST INFRASTRUCTURE ONLY - torch fp32 autograd restatement of the reference's DiscreteBCQ path on the Atari trunk.

Never imported by the product (`tianshou_amd/`).  Lives under tests/ next to the tests that use it; the buffer arithmetic and
the Adam step come from oracle/oracle.py and oracle/oracle_dqn.py.

Follows:
  net       two DiscreteActor(preprocess_net, hidden_sizes=[512], softmax_output=False) heads on ONE
            DQNet(features_only=True) trunk (examples/offline/atari_bcq.py:100-118)
  policy    DiscreteBCQPolicy.forward imitation/discrete_bcq.py:104-127: ratio = logits - max logits, mask = ratio < log tau
            (float32), act = argmax(q - FLT_MAX * mask)
  target    DiscreteBCQ._target_q discrete_bcq.py:228-234: act from the live pair, value from the lagged Q network
  update    DiscreteBCQ._update_with_batch discrete_bcq.py:236-261: lagged refresh at iter % freq == 0, smooth_l1 + nll +
            penalty * mean(logits^2), ONE Adam over the 14 tensors (oracle_dqn._adam)
Tensors follow the parameters' device, so the same code is the eager baseline of bench_bcq.py on a GPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle as O
from oracle import oracle_dqn as OD

# DiscreteBCQPolicy.named_parameters(): the shared trunk once (under the model), the Q head, the imitator head
PARAM_ORDER = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b",
               "q1.w", "q1.b", "q2.w", "q2.b", "i1.w", "i1.b", "i2.w", "i2.b"]
LAGGED_ORDER = PARAM_ORDER[:10]            # model_old = a copy of policy.model: its own trunk, no imitator
TIANSHOU_KEYS = ["model.preprocess.net.0.weight", "model.preprocess.net.0.bias", "model.preprocess.net.2.weight",
                 "model.preprocess.net.2.bias", "model.preprocess.net.4.weight", "model.preprocess.net.4.bias",
                 "model.last.model.0.weight", "model.last.model.0.bias", "model.last.model.2.weight", "model.last.model.2.bias",
                 "imitator.last.model.0.weight", "imitator.last.model.0.bias", "imitator.last.model.2.weight",
                 "imitator.last.model.2.bias"]
HIDDEN = 512
FLT_MAX = float(torch.finfo(torch.float32).max)


@dataclass
class BCQConfig:
    gamma: float = 0.99
    n_step: int = 1
    target_update_freq: int = 8000
    unlikely_action_threshold: float = 0.3
    imitation_logits_penalty: float = 1e-2
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    max_grad_norm: float | None = None

    def dqn(self) -> OD.DQNConfig:
        return OD.DQNConfig(gamma=self.gamma, n_step=self.n_step, target_update_freq=self.target_update_freq,
                            lr=self.lr, betas=self.betas, adam_eps=self.adam_eps, max_grad_norm=self.max_grad_norm)

    def log_tau(self) -> float:
        t = self.unlikely_action_threshold
        return math.log(t) if t > 0 else -math.inf


def feature_dim(h: int, w: int) -> int:
    oh, ow = OD.conv_out_hw(h, w)[-1]
    return 64 * oh * ow


def init_params(c: int, h: int, w: int, n_act: int, seed: int = 0) -> dict[str, torch.Tensor]:
    """Same RNG consumption as `torch.manual_seed(seed)` + the example's construction: the DQNet trunk, the model's MLP, the
    imitator's MLP (tools/gen_golden_bcq.py asserts the equality tensor by tensor)."""
    torch.manual_seed(seed)
    f = feature_dim(h, w)
    mods = {"conv1": torch.nn.Conv2d(c, 32, 8, 4), "conv2": torch.nn.Conv2d(32, 64, 4, 2), "conv3": torch.nn.Conv2d(64, 64, 3, 1),
            "q1": torch.nn.Linear(f, HIDDEN), "q2": torch.nn.Linear(HIDDEN, n_act),
            "i1": torch.nn.Linear(f, HIDDEN), "i2": torch.nn.Linear(HIDDEN, n_act)}
    p = {}
    for name, m in mods.items():
        p[name + ".w"] = m.weight.detach().clone()
        p[name + ".b"] = m.bias.detach().clone()
    return p


def features(p, obs) -> torch.Tensor:
    dev = p["conv1.w"].device
    x = torch.as_tensor(np.asarray(obs) if not isinstance(obs, torch.Tensor) else obs).to(dev, torch.float32)
    x = F.relu(F.conv2d(x, p["conv1.w"], p["conv1.b"], stride=4))
    x = F.relu(F.conv2d(x, p["conv2.w"], p["conv2.b"], stride=2))
    x = F.relu(F.conv2d(x, p["conv3.w"], p["conv3.b"], stride=1))
    return x.flatten(1)


def head(p, feat, which: str) -> torch.Tensor:
    return F.linear(F.relu(F.linear(feat, p[which + "1.w"], p[which + "1.b"])), p[which + "2.w"], p[which + "2.b"])


def masked_argmax(q: torch.Tensor, logits: torch.Tensor, log_tau: float) -> torch.Tensor:
    """discrete_bcq.py:116-118, float32 as the reference (the Python float log_tau meets a float32 tensor)."""
    ratio = logits - logits.max(dim=-1, keepdim=True).values
    mask = (ratio < log_tau).float()
    return (q - FLT_MAX * mask).argmax(dim=-1)


def policy_forward(p, obs, log_tau: float):
    """DiscreteBCQPolicy.forward -> (q [B, A], logits [B, A], act [B])."""
    feat = features(p, obs)
    q, lg = head(p, feat, "q"), head(p, feat, "i")
    return q, lg, masked_argmax(q, lg, log_tau)


def target_q(st: OD.DQNState, cfg: BCQConfig, obs_next, want_act: bool = False):
    """discrete_bcq.py:228-234 -> [B] (and the action)."""
    with torch.no_grad():
        _, _, act = policy_forward(st.params, obs_next, cfg.log_tau())
        tq = head(st.params_old, features(st.params_old, obs_next), "q")
        out = tq[torch.arange(len(act)), act]
    return (out, act) if want_act else out


def preprocess(st: OD.DQNState, cfg: BCQConfig, bstate: O.BufferState, frames: np.ndarray, indices, stack_num: int = 1,
               obs_next_frames: np.ndarray | None = None, acts: list | None = None) -> np.ndarray:
    """discrete_bcq.py:213-226 -> returns float32 [I]; `acts` collects the target pass's actions."""

    def tq_fn(after):
        if obs_next_frames is None:
            on = OD.stacked_frames(bstate, frames, bstate.next(after), stack_num)
        else:
            on = OD.stacked_frames(bstate, obs_next_frames, after, stack_num)
        out, act = target_q(st, cfg, on, want_act=True)
        if acts is not None:
            acts.append(act.cpu().numpy())
        return out.cpu().numpy().reshape(-1, 1)

    ret, _ = O.compute_nstep_return(bstate, indices, tq_fn, cfg.gamma, cfg.n_step)
    return ret.astype(np.float32).reshape(-1)


def loss_terms(p, cfg: BCQConfig, obs, act, returns):
    """discrete_bcq.py:244-252 -> (loss, q_loss, i_loss, reg_loss: scalar tensors with graph, q [B, A], logits [B, A])."""
    feat = features(p, obs)
    dev = feat.device
    q, lg = head(p, feat, "q"), head(p, feat, "i")
    act_t = torch.as_tensor(np.asarray(act.cpu()) if isinstance(act, torch.Tensor) else np.asarray(act), dtype=torch.int64, device=dev)
    target = torch.as_tensor(returns, dtype=torch.float32, device=dev).flatten()
    current_q = q[torch.arange(len(target), device=dev), act_t]
    q_loss = F.smooth_l1_loss(current_q, target)
    i_loss = F.nll_loss(F.log_softmax(lg, dim=-1), act_t)
    reg_loss = lg.pow(2).mean()
    loss = q_loss + i_loss + cfg.imitation_logits_penalty * reg_loss
    return loss, q_loss, i_loss, reg_loss, q, lg


def make_state(p, cfg: BCQConfig) -> OD.DQNState:
    st = OD.DQNState.create(p, cfg.dqn())
    st.params_old = {k: p[k].clone() for k in LAGGED_ORDER}
    return st


def update_with_batch(st: OD.DQNState, cfg: BCQConfig, obs, act, returns, collect: dict | None = None):
    """discrete_bcq.py:236-261 -> (loss, q_loss, i_loss, reg_loss) floats."""
    if st.iter % cfg.target_update_freq == 0:
        st.params_old = {k: st.params[k].clone() for k in LAGGED_ORDER}
    st.iter += 1
    p = {k: v.clone().requires_grad_(True) for k, v in st.params.items()}
    loss, q_loss, i_loss, reg_loss, q, lg = loss_terms(p, cfg, obs, act, returns)
    loss.backward()
    grads = {k: v.grad for k, v in p.items()}
    if collect is not None:
        collect["q"], collect["logits"] = q.detach().clone(), lg.detach().clone()
        collect["grads"] = {k: g.clone() for k, g in grads.items()}
    OD._adam(st, cfg.dqn(), grads)
    return tuple(float(x.item()) for x in (loss, q_loss, i_loss, reg_loss))
