"""TEST INFRASTRUCTURE ONLY - torch fp32 autograd restatement of the reference's IQN path on the Atari trunk.

Never imported by the product (`tianshou_amd/`).  Lives under tests/ next to the tests that use it; the trunk helpers
come from oracle/oracle_dqn.py.  Every function takes the fractions `tau` as inputs (the reference draws them with
torch.rand inside ImplicitQuantileNetwork.forward, utils/net/discrete.py:210).

Follows:
  net       ImplicitQuantileNetwork.forward utils/net/discrete.py:200-216 with preprocess_net = DQNet(features_only=True)
            (env/atari/atari_network.py:79-122) and hidden_sizes = [512]; CosineEmbeddingNetwork.forward :144-160
  policy    IQNPolicy.forward modelfree/iqn.py:72-100 (Q = mean over the fractions, qrdqn.py:19-21; act = argmax)
  target    QRDQN._target_q qrdqn.py:94-106 (online sample size for the action, target sample size for the quantiles)
  update    IQN._update_with_batch iqn.py:156-183, periodic hard sync dqn.py:277-285, Optimizer.step
            algorithm_base.py:484-500 (oracle_dqn._adam)
Tensors follow the parameters' device, so the same code is the eager baseline of bench_iqn.py on a GPU.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle as O
from oracle import oracle_dqn as OD

warnings.filterwarnings("ignore", message="Using a target size")      # as qrdqn.py:92: the broadcast is intended

# state_dict order of the reference net: preprocess.net.{0,2,4}, last.model.{0,2}, embed_model.net.0
PARAM_ORDER = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b",
               "fc1.w", "fc1.b", "fc2.w", "fc2.b", "emb.w", "emb.b"]
TIANSHOU_KEYS = ["preprocess.net.0.weight", "preprocess.net.0.bias", "preprocess.net.2.weight", "preprocess.net.2.bias",
                 "preprocess.net.4.weight", "preprocess.net.4.bias", "last.model.0.weight", "last.model.0.bias",
                 "last.model.2.weight", "last.model.2.bias", "embed_model.net.0.weight", "embed_model.net.0.bias"]
HIDDEN = 512


@dataclass
class IQNConfig:
    n_cos: int = 64
    sample_size: int = 32
    online_sample_size: int = 8
    target_sample_size: int = 8
    gamma: float = 0.99
    n_step: int = 1
    target_update_freq: int = 0
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    max_grad_norm: float | None = None

    def dqn(self) -> OD.DQNConfig:
        return OD.DQNConfig(gamma=self.gamma, n_step=self.n_step, target_update_freq=self.target_update_freq,
                            lr=self.lr, betas=self.betas, adam_eps=self.adam_eps, max_grad_norm=self.max_grad_norm)


def feature_dim(h: int, w: int) -> int:
    oh, ow = OD.conv_out_hw(h, w)[-1]
    return 64 * oh * ow


def param_shapes(c: int, h: int, w: int, n_act: int, n_cos: int = 64) -> dict[str, tuple[int, ...]]:
    f = feature_dim(h, w)
    return {"conv1.w": (32, c, 8, 8), "conv1.b": (32,), "conv2.w": (64, 32, 4, 4), "conv2.b": (64,),
            "conv3.w": (64, 64, 3, 3), "conv3.b": (64,), "fc1.w": (HIDDEN, f), "fc1.b": (HIDDEN,),
            "fc2.w": (n_act, HIDDEN), "fc2.b": (n_act,), "emb.w": (f, n_cos), "emb.b": (f,)}


def init_params(c: int, h: int, w: int, n_act: int, n_cos: int = 64, seed: int = 0) -> dict[str, torch.Tensor]:
    """Same RNG consumption as `torch.manual_seed(seed)` + the reference's construction (DQNet trunk, the critic's MLP, the
    embedding; tools/gen_golden_iqn.py asserts the equality tensor by tensor)."""
    torch.manual_seed(seed)
    f = feature_dim(h, w)
    mods = {"conv1": torch.nn.Conv2d(c, 32, 8, 4), "conv2": torch.nn.Conv2d(32, 64, 4, 2), "conv3": torch.nn.Conv2d(64, 64, 3, 1),
            "fc1": torch.nn.Linear(f, HIDDEN), "fc2": torch.nn.Linear(HIDDEN, n_act), "emb": torch.nn.Linear(n_cos, f)}
    p = {}
    for name, m in mods.items():
        p[name + ".w"] = m.weight.detach().clone()
        p[name + ".b"] = m.bias.detach().clone()
    return p


def features(p, obs) -> torch.Tensor:
    """DQNet(features_only=True).forward: obs u8/f32 [B, C, H, W] -> [B, F] in torch's (c, h, w) order."""
    dev = p["conv1.w"].device
    x = torch.as_tensor(np.asarray(obs) if not isinstance(obs, torch.Tensor) else obs).to(dev, torch.float32)
    x = F.relu(F.conv2d(x, p["conv1.w"], p["conv1.b"], stride=4))
    x = F.relu(F.conv2d(x, p["conv2.w"], p["conv2.b"], stride=2))
    x = F.relu(F.conv2d(x, p["conv3.w"], p["conv3.b"], stride=1))
    return x.flatten(1)


def embed(p, taus: torch.Tensor) -> torch.Tensor:
    """CosineEmbeddingNetwork.forward (discrete.py:144-160): taus [B, N] -> [B, N, F]."""
    b, n = taus.shape
    k = p["emb.w"].shape[1]
    i_pi = np.pi * torch.arange(start=1, end=k + 1, dtype=taus.dtype, device=taus.device).view(1, 1, k)
    cosines = torch.cos(taus.view(b, n, 1) * i_pi).view(b * n, k)
    return F.relu(F.linear(cosines, p["emb.w"], p["emb.b"])).view(b, n, -1)


def logits(p, obs, taus) -> torch.Tensor:
    """ImplicitQuantileNetwork.forward (discrete.py:200-216) -> [B, A, N]."""
    feat = features(p, obs)
    taus = torch.as_tensor(taus, dtype=torch.float32, device=feat.device)
    b, n = taus.shape
    x = (feat.unsqueeze(1) * embed(p, taus)).view(b * n, -1)
    out = F.linear(F.relu(F.linear(x, p["fc1.w"], p["fc1.b"])), p["fc2.w"], p["fc2.b"])
    return out.view(b, n, -1).transpose(1, 2)


def policy_forward(p, obs, taus):
    """IQNPolicy.forward (iqn.py:72-100) -> (logits [B, A, N], q [B, A], act [B])."""
    lg = logits(p, obs, taus)
    q = lg.mean(2)
    return lg, q, q.max(dim=1)[1]


def next_dist(st: OD.DQNState, obs_next, tau_online, tau_target=None) -> torch.Tensor:
    """qrdqn.py:94-106 -> [B, N'] ([B, N] without a target network)."""
    with torch.no_grad():
        lg, _, act = policy_forward(st.params, obs_next, tau_online)
        if st.params_old is not None:
            lg = logits(st.params_old, obs_next, tau_target)
        return lg[torch.arange(len(act)), act, :]


def preprocess(st: OD.DQNState, cfg: IQNConfig, bstate: O.BufferState, frames: np.ndarray, indices, tau_online,
               tau_target=None, stack_num: int = 1, obs_next_frames: np.ndarray | None = None) -> np.ndarray:
    """QLearningOffPolicyAlgorithm._preprocess_batch (dqn.py:257-275) -> returns float32 [I, N']."""

    def tq_fn(after):
        if obs_next_frames is None:
            on = OD.stacked_frames(bstate, frames, bstate.next(after), stack_num)
        else:
            on = OD.stacked_frames(bstate, obs_next_frames, after, stack_num)
        return next_dist(st, on, tau_online, tau_target).cpu().numpy()

    ret, _ = O.compute_nstep_return(bstate, indices, tq_fn, cfg.gamma, cfg.n_step)
    return ret.astype(np.float32)


def loss_terms(p, obs, act, returns, taus, weight=None):
    """iqn.py:162-180 -> (loss scalar tensor with graph, new batch.weight [B], logits [B, A, N])."""
    lg = logits(p, obs, taus)
    dev = lg.device
    act_t = torch.as_tensor(np.asarray(act.cpu()) if isinstance(act, torch.Tensor) else np.asarray(act), dtype=torch.int64, device=dev)
    ret = torch.as_tensor(returns, dtype=torch.float32, device=dev)
    taus = torch.as_tensor(taus, dtype=torch.float32, device=dev)
    w = 1.0 if weight is None else torch.as_tensor(weight, dtype=torch.float32, device=dev)
    curr = lg[torch.arange(len(act_t), device=dev), act_t, :].unsqueeze(2)
    tgt = ret.unsqueeze(1)
    dist_diff = F.smooth_l1_loss(tgt, curr, reduction="none")
    huber = (dist_diff * (taus.unsqueeze(2) - (tgt - curr).detach().le(0.0).float()).abs()).sum(-1).mean(1)
    loss = (huber * w).mean()
    prio = dist_diff.detach().abs().sum(-1).mean(1)
    return loss, prio, lg


def update_with_batch(st: OD.DQNState, cfg: IQNConfig, obs, act, returns, taus, weight=None, collect: dict | None = None):
    """iqn.py:156-183 -> (loss float, new batch.weight float32[B])."""
    if st.params_old is not None and st.iter % cfg.target_update_freq == 0:      # dqn.py:283-285
        st.params_old = {k: v.clone() for k, v in st.params.items()}
    st.iter += 1
    p = {k: v.clone().requires_grad_(True) for k, v in st.params.items()}
    loss, prio, lg = loss_terms(p, obs, act, returns, taus, weight)
    loss.backward()
    grads = {k: v.grad for k, v in p.items()}
    if collect is not None:
        collect["logits"] = lg.detach().clone()
        collect["grads"] = {k: g.clone() for k, g in grads.items()}
    OD._adam(st, cfg.dqn(), grads)
    return float(loss.item()), prio.clone()
