"""TEST INFRASTRUCTURE ONLY - float64 torch reference of IQN on the plain MLP Net: ImplicitQuantileNetwork.forward and
CosineEmbeddingNetwork.forward (utils/net/discrete.py:144-216), QRDQN._target_q and one IQN._update_with_batch + Adam step
(modelfree/qrdqn.py:94-106, iqn.py:156-183; torch.optim.Adam's single-tensor formulas).  `layers` = (obs_dim, trunk, feat, C, H, A)
as tianshou_amd.iqn_mlp takes it; parameters are a dict in state_dict() order.  The fractions are inputs.  The cosine ARGUMENT is
formed in float32 as torch forms it (tau * fl32(pi * (k + 1))); everything else runs in `dtype` (float32: the measure of what
float32 can resolve)."""
import numpy as np
import torch

from tests.oracle_qrdqn_mlp import Agent as _QRAgent


def shapes(layers):
    obs_dim, trunk, feat, n_cos, hidden, n_act = layers
    out, k = {}, obs_dim
    for i, n in enumerate(tuple(trunk) + ((feat,) if feat else ())):
        out[f"preprocess.model.model.{2 * i}.weight"], out[f"preprocess.model.model.{2 * i}.bias"] = (n, k), (n,)
        k = n
    f = k
    for i, n in enumerate(tuple(hidden) + (n_act,)):
        out[f"last.model.{2 * i}.weight"], out[f"last.model.{2 * i}.bias"] = (n, k), (n,)
        k = n
    out["embed_model.net.0.weight"], out["embed_model.net.0.bias"] = (f, n_cos), (f,)
    return out


def init_params(layers, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shp in shapes(layers).items():
        bound = scale / (shp[-1] if k.endswith("weight") else out[k[:-4] + "weight"].shape[1]) ** 0.5
        out[k] = (torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) * bound
    return out


def forward(params, layers, obs, tau, want_pre=False, dtype=torch.float64):
    """-> logits [B, A, N] (and every ReLU pre-activation as [B, *] tensors: trunk, embedding, `last`)."""
    _, trunk, feat, n_cos, hidden, _ = layers
    lin = lambda x, name: x @ params[name + ".weight"].to(dtype).t() + params[name + ".bias"].to(dtype)  # noqa: E731
    x, pre = obs.to(dtype), []
    for i in range(len(trunk)):
        z = lin(x, f"preprocess.model.model.{2 * i}")
        pre.append(z)
        x = torch.relu(z)
    if feat:
        x = lin(x, f"preprocess.model.model.{2 * len(trunk)}")
    b, n = tau.shape
    i_pi = np.pi * torch.arange(start=1, end=n_cos + 1, dtype=torch.float32).view(1, 1, n_cos)
    cos = torch.cos((tau.float().view(b, n, 1) * i_pi).to(dtype))
    z = lin(cos, "embed_model.net.0")
    pre.append(z.reshape(b, -1))
    x = x.unsqueeze(1) * torch.relu(z)
    for i in range(len(hidden)):
        z = lin(x, f"last.model.{2 * i}")
        pre.append(z.reshape(b, -1))
        x = torch.relu(z)
    out = lin(x, f"last.model.{2 * len(hidden)}").transpose(1, 2)
    return (out, pre) if want_pre else out


class Agent(_QRAgent):
    """tests/oracle_qrdqn_mlp.Agent's state, Adam and clipping over this network; every method takes the fractions."""

    def __init__(self, params, layers, **kw):
        kw.pop("is_double", None)
        super().__init__(params, (0, (), 0, 1), **kw)
        self.layers = layers

    def next_dist(self, obs_next, tau_online, tau_target=None):
        """qrdqn.py:94-106 -> [B, N'] ([B, N] without a lagged network)."""
        lg = forward(self.params, self.layers, obs_next, tau_online)
        act = lg.mean(2).max(dim=1)[1]
        if self.old is not None:
            lg = forward(self.old, self.layers, obs_next, tau_target)
        return lg[torch.arange(len(act)), act]

    def loss(self, params, obs, act, returns, weight, tau, dtype=torch.float64):
        """iqn.py:162-180 -> (loss, new priorities)."""
        curr = forward(params, self.layers, obs, tau, dtype=dtype)[torch.arange(len(act)), act].unsqueeze(2)
        target = returns.to(dtype).unsqueeze(1)
        diff = torch.nn.functional.smooth_l1_loss(target.expand(-1, curr.shape[1], -1), curr.expand(-1, -1, target.shape[2]), reduction="none")
        huber = (diff * (tau.to(dtype).unsqueeze(2) - (target - curr).detach().le(0.0).to(dtype)).abs()).sum(-1).mean(1)
        w = 1.0 if weight is None else weight.to(dtype)
        return (huber * w).mean(), diff.detach().abs().sum(-1).mean(1)

    def gradient(self, obs, act, returns, weight=None, tau=None):
        p = {k: t.clone().requires_grad_(True) for k, t in self.params.items()}
        loss, prio = self.loss(p, obs, act, returns, weight, tau)
        return dict(zip(p, torch.autograd.grad(loss, list(p.values())))), loss.detach(), prio

    def update(self, obs, act, returns, weight=None, tau=None):
        """iqn.py:156-183 -> (loss, new priorities): the sibling's sync, clipping and Adam over this gradient."""
        grad = self.gradient
        self.gradient = lambda o, a, r, w=None: grad(o, a, r, w, tau)
        try:
            return super().update(obs, act, returns, weight)
        finally:
            del self.gradient
