"""TEST INFRASTRUCTURE ONLY - float64 torch reference of QRDQN on the plain MLP Net with `num_atoms` quantiles per action:
Net.forward (utils/net/common.py:343-369), QRDQNPolicy.compute_q_value, QRDQN._target_q and one _update_with_batch + Adam step
(modelfree/qrdqn.py:19-21, 94-131; torch.optim.Adam's single-tensor formulas).  `layers` = (obs_dim, trunk, n_act, n_atoms) as
tianshou_amd.qrdqn_mlp takes it; parameters are a dict in Net.state_dict() order.  `dtype` float32 evaluates the same formulas
in float32 (the measure of what float32 can resolve)."""
import torch

from tests import oracle_dqn_mlp as OM


def plain(layers):
    obs_dim, trunk, n_act, n_atoms = layers
    return (obs_dim, trunk, None, None, n_act * n_atoms)


def init_params(layers, seed, scale=1.0):
    return OM.init_params(plain(layers), seed, scale)


def forward(params, layers, obs, want_pre=False, dtype=torch.float64):
    """-> dist [B, A, N] (and every ReLU pre-activation, for the input-selection rule)."""
    x, pre = obs.to(dtype), []
    for i in range(len(layers[1])):
        z = x @ params[f"model.model.{2 * i}.weight"].to(dtype).t() + params[f"model.model.{2 * i}.bias"].to(dtype)
        pre.append(z)
        x = torch.relu(z)
    n = 2 * len(layers[1])
    dist = (x @ params[f"model.model.{n}.weight"].to(dtype).t() + params[f"model.model.{n}.bias"].to(dtype)).view(len(obs), layers[2], layers[3])
    return (dist, pre) if want_pre else dist


class Agent:
    def __init__(self, params, layers, *, target_update_freq=0, is_double=True, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        self.layers, self.freq, self.is_double, self.lr, self.betas, self.eps, self.clip = layers, target_update_freq, is_double, lr, betas, eps, max_grad_norm
        self.params = {k: p.detach().to(torch.float64).clone() for k, p in params.items()}
        self.old = {k: p.clone() for k, p in self.params.items()} if target_update_freq > 0 else None
        self.m = {k: torch.zeros_like(p) for k, p in self.params.items()}
        self.v = {k: torch.zeros_like(p) for k, p in self.params.items()}
        self.step = self.iter = 0
        tau = torch.linspace(0, 1, layers[3] + 1)                      # qrdqn.py:87-91, float32 as the reference holds it
        self.tau_hat = ((tau[:-1] + tau[1:]) / 2).view(1, -1, 1)

    def target_dist(self, obs_next):
        """qrdqn.py:94-106 (`is_double` False: the lagged network selects for itself)."""
        new = forward(self.params, self.layers, obs_next)
        old = forward(self.old, self.layers, obs_next) if self.old is not None else new
        act = (new if self.is_double else old).mean(2).max(dim=1)[1]
        return old[torch.arange(len(act)), act]

    def loss(self, params, obs, act, returns, weight, dtype=torch.float64):
        """qrdqn.py:114-128 -> (loss, new priorities)."""
        curr = forward(params, self.layers, obs, dtype=dtype)[torch.arange(len(act)), act].unsqueeze(2)
        target = returns.to(dtype).unsqueeze(1)
        diff = torch.nn.functional.smooth_l1_loss(target.expand(-1, curr.shape[1], -1), curr.expand(-1, -1, target.shape[2]), reduction="none")
        huber = (diff * (self.tau_hat.to(dtype) - (target - curr).detach().le(0.0).to(dtype)).abs()).sum(-1).mean(1)
        w = 1.0 if weight is None else weight.to(dtype)
        return (huber * w).mean(), diff.detach().abs().sum(-1).mean(1)

    def gradient(self, obs, act, returns, weight=None):
        p = {k: t.clone().requires_grad_(True) for k, t in self.params.items()}
        loss, prio = self.loss(p, obs, act, returns, weight)
        return dict(zip(p, torch.autograd.grad(loss, list(p.values())))), loss.detach(), prio

    def update(self, obs, act, returns, weight=None):
        """qrdqn.py:108-131 -> (loss, new priorities)."""
        if self.old is not None and self.iter % self.freq == 0:
            self.old = {k: p.clone() for k, p in self.params.items()}
        self.iter += 1
        grad, loss, prio = self.gradient(obs, act, returns, weight)
        if self.clip:                                                   # clip_grad_norm_ (algorithm_base.py:496-500)
            norm = torch.sqrt(sum(g.pow(2).sum() for g in grad.values()))
            grad = {k: g * torch.clamp(self.clip / (norm + 1e-6), max=1.0) for k, g in grad.items()}
        self.step += 1
        b1, b2 = self.betas
        for k, g in grad.items():
            self.m[k] = self.m[k] + (g - self.m[k]) * (1 - b1)
            self.v[k] = self.v[k] * b2 + (1 - b2) * g * g
            denom = self.v[k].sqrt() / (1 - b2 ** self.step) ** 0.5 + self.eps
            self.params[k] = self.params[k] - (self.lr / (1 - b1 ** self.step)) * self.m[k] / denom
        return loss, prio
