"""TEST INFRASTRUCTURE ONLY - float64 torch reference of FQF on the plain MLP Net, on tests/oracle_iqn_mlp.py's walk:
FractionProposalNetwork.forward (utils/net/discrete.py:239-252), FQFPolicy.forward's weighted q (modelfree/fqf.py:94-98), FQF._target_q
(fqf.py:178-193) and one FQF._update_with_batch (fqf.py:195-256) with both losses as the reference writes them, gradients by autograd
and the two steps by torch.optim (foreach=False).  The walks take the fractions as inputs, so a test can feed them the engine's own
float32 taus / tau_hats: the cosines multiply a fraction error by up to 64 pi.  The fraction loss's gradient flows through the oracle's
own float64 proposal."""
import torch
import torch.nn.functional as F

from tests import oracle_iqn_mlp as OI
from tests.oracle_iqn_mlp import init_params  # noqa: F401


def init_fraction_params(feat, n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * scale / feat ** 0.5  # noqa: E731
    return {"net.weight": u(n, feat), "net.bias": u(n)}


def features(params, layers, obs, dtype=torch.float64):
    _, trunk, feat, *_ = layers
    x = obs.to(dtype)
    for i in range(len(trunk) + bool(feat)):
        x = x @ params[f"preprocess.model.model.{2 * i}.weight"].to(dtype).t() + params[f"preprocess.model.model.{2 * i}.bias"].to(dtype)
        x = torch.relu(x) if i < len(trunk) else x
    return x


def propose(fparams, feats, dtype=torch.float64):
    """discrete.py:239-252 -> (taus [B, N + 1], tau_hats [B, N], entropies [B])."""
    dist = torch.distributions.Categorical(logits=feats.detach().to(dtype) @ fparams["net.weight"].to(dtype).t() + fparams["net.bias"].to(dtype))
    taus = F.pad(torch.cumsum(dist.probs, dim=1), (1, 0))
    return taus, (taus[:, :-1] + taus[:, 1:]).detach() / 2.0, dist.entropy()


def weighted_q(logits, taus):
    """fqf.py:94-96."""
    return ((taus[:, 1:] - taus[:, :-1]).unsqueeze(1).to(logits.dtype) * logits).sum(2)


def tau_gradient(hat, th):
    """fqf.py:227-243 -> (gradient_of_taus [B, N - 1], the smallest distance between the two sides of any of its comparisons)."""
    left, right = torch.cat([hat[:, :1], th[:, :-1]], dim=1), torch.cat([th[:, 1:], hat[:, -1:]], dim=1)
    v1, v2 = th - hat[:, :-1], th - hat[:, 1:]
    g = torch.where(th > left, v1, -v1) + torch.where(th < right, v2, -v2)
    return g, torch.minimum((th - left).abs(), (th - right).abs()).min(dim=1)[0]


class Agent:
    def __init__(self, params, fparams, layers, *, target_update_freq=0, lr=1e-3, max_grad_norm=None, ent_coef=0.0, f_optim="rmsprop",
                 f_lr=1e-3):
        leaf = lambda d: {k: p.detach().to(torch.float64).clone().requires_grad_(True) for k, p in d.items()}  # noqa: E731
        self.layers, self.freq, self.clip, self.ent_coef = layers, target_update_freq, max_grad_norm, ent_coef
        self.params, self.fparams = leaf(params), leaf(fparams)
        self.old = {k: p.detach().clone() for k, p in self.params.items()} if target_update_freq > 0 else None
        self.optim = torch.optim.Adam(list(self.params.values()), lr=lr, foreach=False)
        self.f_optim = (torch.optim.RMSprop if f_optim == "rmsprop" else torch.optim.Adam)(list(self.fparams.values()), lr=f_lr, foreach=False)
        self.iter = 0

    def fractions(self, obs):
        with torch.no_grad():
            return propose(self.fparams, features(self.params, self.layers, obs))

    def next_dist(self, obs_next, taus, tau_hats):
        """fqf.py:178-193 on the given fractions -> [B, N]."""
        with torch.no_grad():
            lg = OI.forward(self.params, self.layers, obs_next, tau_hats)
            act = weighted_q(lg, taus).max(dim=1)[1]
            if self.old is not None:
                lg = OI.forward(self.old, self.layers, obs_next, tau_hats)
            return lg[torch.arange(len(act)), act]

    def losses(self, obs, act, returns, weight, taus_in, tau_hats_in):
        """fqf.py:200-247 -> (quantile_loss, fraction_loss, entropy_loss, new priorities, the comparisons' smallest gap per row)."""
        r = torch.arange(len(act))
        taus, _, ent = propose(self.fparams, features(self.params, self.layers, obs))
        curr = OI.forward(self.params, self.layers, obs, tau_hats_in)[r, act]
        with torch.no_grad():
            g, gap = tau_gradient(curr.detach(), OI.forward(self.params, self.layers, obs, taus_in[:, 1:-1])[r, act])
        target = returns.double().unsqueeze(1)
        c = curr.unsqueeze(2)
        diff = F.smooth_l1_loss(target.expand(-1, c.shape[1], -1), c.expand(-1, -1, target.shape[2]), reduction="none")
        huber = (diff * (tau_hats_in.double().unsqueeze(2) - (target - c).detach().le(0.0).double()).abs()).sum(-1).mean(1)
        w = 1.0 if weight is None else weight.double()
        return (huber * w).mean(), (g * taus[:, 1:-1]).sum(1).mean(), ent.mean(), diff.detach().abs().sum(-1).mean(1), gap

    def gradient(self, obs, act, returns, weight, taus, tau_hats):
        """-> ({model gradients}, {fraction gradients}, (three losses), prio)."""
        ql, fl, el, prio, _ = self.losses(obs, act, returns, weight, taus, tau_hats)
        grad = torch.autograd.grad(ql, list(self.params.values()), retain_graph=True)
        fgrad = torch.autograd.grad(fl - self.ent_coef * el, list(self.fparams.values()))
        return dict(zip(self.params, grad)), dict(zip(self.fparams, fgrad)), torch.stack([ql, fl, el]).detach(), prio

    def update(self, obs, act, returns, weight, taus, tau_hats):
        """fqf.py:195-256 -> (three losses, new priorities)."""
        if self.old is not None and self.iter % self.freq == 0:
            self.old = {k: p.detach().clone() for k, p in self.params.items()}
        self.iter += 1
        grad, fgrad, losses, prio = self.gradient(obs, act, returns, weight, taus, tau_hats)
        if self.clip:                                                   # clip_grad_norm_ (algorithm_base.py:496-500)
            norm = torch.sqrt(sum(g.pow(2).sum() for g in grad.values()))
            grad = {k: g * torch.clamp(self.clip / (norm + 1e-6), max=1.0) for k, g in grad.items()}
        for d, g in ((self.params, grad), (self.fparams, fgrad)):
            for k, p in d.items():
                p.grad = g[k]
        self.f_optim.step()
        self.optim.step()
        return losses, prio
