"""TEST INFRASTRUCTURE ONLY - a torch oracle of Branching DQN written from its formulas (arXiv 1711.08946 as the reference
configures it); no reference import.  Works in the dtype of the tensors it is given (float32 on either device, float64).

Network (`dims` = (obs_dim, common_hidden, value_hidden, action_hidden, D, A, activation); a hidden width of 0 = no hidden layer):
    h = common(obs): Linear + activation per layer, the last hidden layer is the output
    v = value(h) [B, 1];  adv[b, d, :] = branches[d](h) [A];  q[b, d, a] = v[b] + (adv[b, d, a] - mean_a adv[b, d, :])
Target (1-step):  a*[b, d] = argmax_a q_sel[b, d, :] (lowest index on ties);
    ret[b] = rew[b] + gamma mean_d q_eval[b, d, a*[b, d]] (1 - end[b])
    q_sel = online Q(s') when is_double, otherwise q_eval; q_eval = lagged Q(s') when there is a lagged network, otherwise online.
Loss:  td[b, d] = ret[b] - q[b, d, act[b, d]];  loss = mean_b(w[b] mean_d td^2);  prio[b] = sum_d td[b, d] (signed).
The lagged network is synchronised at the START of every target_update_freq-th update (the first included), after that update's
target was computed.  An action outside [0, A) is clamped into it (the engine's convention).
"""
from __future__ import annotations

import torch


def state_keys(dims) -> list[str]:
    _, ch, hv, ha, d_n, _, _ = dims
    pre = [f"common.model.{2 * i}" for i in range(len(ch))]
    pre += ["value.model.0"] + (["value.model.2"] if hv else [])
    for d in range(d_n):
        pre += [f"branches.{d}.model.0"] + ([f"branches.{d}.model.2"] if ha else [])
    return [f"{p}.{s}" for p in pre for s in ("weight", "bias")]


def shapes(dims) -> dict:
    """key -> shape, nn.Linear layout."""
    obs_dim, ch, hv, ha, d_n, a_n, _ = dims
    out, k = {}, obs_dim

    def lin(prefix, k, n):
        out[f"{prefix}.weight"], out[f"{prefix}.bias"] = (n, k), (n,)

    for i, n in enumerate(ch):
        lin(f"common.model.{2 * i}", k, n)
        k = n
    if hv:
        lin("value.model.0", k, hv)
        lin("value.model.2", hv, 1)
    else:
        lin("value.model.0", k, 1)
    for d in range(d_n):
        if ha:
            lin(f"branches.{d}.model.0", k, ha)
            lin(f"branches.{d}.model.2", ha, a_n)
        else:
            lin(f"branches.{d}.model.0", k, a_n)
    return {key: out[key] for key in state_keys(dims)}


def random_params(dims, seed: int, dtype=torch.float32, device="cpu", scale: float = 1.0) -> dict:
    """Uniform(-1/sqrt(k), 1/sqrt(k)) like nn.Linear's default, from a seeded CPU generator (the same values in every dtype)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key, shp in shapes(dims).items():
        k = shp[1] if len(shp) == 2 else None
        bound = scale / (k if k is not None else out[key.replace("bias", "weight")].shape[1]) ** 0.5
        out[key] = ((torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) * bound).to(dtype).to(device)
    return out


def _act(dims):
    return torch.relu if dims[6] == "relu" else torch.tanh


def _mlp(params, prefix, x, n_linear, act, pre):
    for i in range(n_linear):
        x = x @ params[f"{prefix}.model.{2 * i}.weight"].t() + params[f"{prefix}.model.{2 * i}.bias"]
        if i + 1 < n_linear:
            if pre is not None:
                pre.append(x)
            x = act(x)
    return x


def forward(params, dims, obs, pre=None):
    """-> q [B, D, A].  `pre`: a list that receives every hidden layer's pre-activation."""
    _, ch, hv, ha, d_n, a_n, _ = dims
    act = _act(dims)
    h = obs
    for i in range(len(ch)):
        z = h @ params[f"common.model.{2 * i}.weight"].t() + params[f"common.model.{2 * i}.bias"]
        if pre is not None:
            pre.append(z)
        h = act(z)
    v = _mlp(params, "value", h, 2 if hv else 1, act, pre).unsqueeze(1)                       # [B, 1, 1]
    adv = torch.stack([_mlp(params, f"branches.{d}", h, 2 if ha else 1, act, pre) for d in range(d_n)], 1)
    return v + (adv - adv.mean(2, keepdim=True))


def argmax_lowest(q):
    """argmax over the last axis, ties to the lowest index."""
    a_n = q.shape[-1]
    idx = torch.arange(a_n, device=q.device).expand(q.shape)
    return torch.where(q == q.max(-1, keepdim=True).values, idx, torch.full_like(idx, a_n)).min(-1).values


def target(q_sel, q_eval, rew, end, gamma: float):
    a = argmax_lowest(q_sel)
    boot = q_eval.gather(-1, a.unsqueeze(-1)).squeeze(-1).mean(-1)
    return rew.to(q_eval.dtype) + gamma * boot * (1.0 - end.to(q_eval.dtype))


def td_errors(q, act, ret):
    a = act.clamp(0, q.shape[-1] - 1)
    return ret.unsqueeze(-1) - q.gather(-1, a.unsqueeze(-1)).squeeze(-1)                      # [B, D]


def loss(q, act, ret, weight=None):
    """-> (loss, prio [B] signed)"""
    td = td_errors(q, act, ret)
    per = td.pow(2).mean(-1)
    return (per * weight).mean() if weight is not None else per.mean(), td.sum(-1)


class Agent:
    """Parameters, lagged copy, optimizer and the update counter; `update` is one BDQN update."""

    def __init__(self, params: dict, dims, *, gamma, target_update_freq=0, is_double=True, optimizer="adam", lr=1e-3, **opt_kw):
        self.dims, self.gamma, self.freq, self.is_double = dims, gamma, int(target_update_freq), bool(is_double)
        self.params = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
        self.old = {k: v.detach().clone() for k, v in params.items()} if self.freq > 0 else None
        cls = {"adam": torch.optim.Adam, "rmsprop": torch.optim.RMSprop}[optimizer]
        self.optim = cls(list(self.params.values()), lr=lr, **opt_kw)
        self.iter = 0

    def q(self, obs, old=False):
        with torch.no_grad():
            return forward(self.old if old else self.params, self.dims, obs)

    def target_q(self, obs_next, rew, end):
        q_online = self.q(obs_next)
        q_eval = self.q(obs_next, old=True) if self.old is not None else q_online
        return target(q_online if self.is_double else q_eval, q_eval, rew, end, self.gamma)

    def gradient(self, obs, act, ret, weight=None):
        """-> ({key: grad}, loss, prio) at unchanged parameters."""
        val, prio = loss(forward(self.params, self.dims, obs), act, ret, weight)
        grads = torch.autograd.grad(val, list(self.params.values()))
        return dict(zip(self.params, grads)), val.detach(), prio.detach()

    def update(self, obs, act, ret, weight=None):
        if self.old is not None and self.iter % self.freq == 0:
            self.old = {k: v.detach().clone() for k, v in self.params.items()}
        self.iter += 1
        val, prio = loss(forward(self.params, self.dims, obs), act, ret, weight)
        self.optim.zero_grad()
        val.backward()
        self.optim.step()
        return val.detach(), prio.detach()

    def cat(self, old=False) -> torch.Tensor:
        src = self.old if old else self.params
        return torch.cat([src[k].detach().reshape(-1) for k in state_keys(self.dims)])

    def moments(self):
        """-> (first, second) moment vectors in key order (Adam: exp_avg / exp_avg_sq; RMSprop: zeros / square_avg)."""
        ms, vs = [], []
        for k in state_keys(self.dims):
            st = self.optim.state[self.params[k]]
            vs.append((st["exp_avg_sq"] if "exp_avg_sq" in st else st["square_avg"]).reshape(-1))
            ms.append((st["exp_avg"] if "exp_avg" in st else torch.zeros_like(self.params[k])).reshape(-1))
        return torch.cat(ms), torch.cat(vs)
