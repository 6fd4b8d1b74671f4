"""CPU: tests/oracle_bdqn.py on the edge-case tables of tests/bdqn_edge_cases.py -- against hand-derived values, against float64
autograd, and float32 against float64 (the kernels are held to the same tables in tests/test_gpu_bdqn_edges.py).

Measured here, float32 oracle against float64 over all SHAPES / LOSSES entries (tolerance of the GPU tests in brackets; each is
below half of it, asserted by `test_float32_oracle_stays_within_half_the_tolerances`):
    q            |diff| <= 0.092 (rtol 1e-5 |ref| + atol 2e-6)      gradient  3.1e-7 max|ref|  [1e-5 max|ref|]
    loss         rel 1.2e-7  [1e-5]                                 priority  7.9e-8 max|td| D  [1e-5 max|td| D]
"""
import numpy as np
import pytest
import torch

from tests import bdqn_common as BC
from tests import bdqn_edge_cases as EC
from tests import oracle_bdqn as OB

SHAPE_NAMES = [s[0] for s in EC.SHAPES]


def test_tables_cover_the_issue_list():
    assert {s[2] for s in EC.SHAPES} >= {1, 2, 63, 65, 257}
    assert {s[1][4] for s in EC.SHAPES} >= {1, 3, 4, 17, 32} and {s[1][5] for s in EC.SHAPES} >= {1, 2, 5, 25, 33, 64}
    assert {(bool(s[1][2]), bool(s[1][3])) for s in EC.SHAPES} == {(False, False), (True, False), (False, True), (True, True)}
    assert all(w % 32 for s in EC.SHAPES for w in (*s[1][1], s[1][2] or 1, s[1][3] or 1))


@pytest.mark.parametrize("case", EC.targets(), ids=lambda c: c["name"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_target_tables(case, dtype):
    got = OB.target(case["q_sel"].to(dtype), case["q_eval"].to(dtype), case["rew"].to(dtype), case["end"], case["gamma"])
    assert torch.equal(got.to(torch.float32), case["want"])


def test_argmax_takes_the_lowest_index():
    q = torch.tensor([[1.0, 7.0, 3.0, 7.0], [5.0, 2.0, 5.0, 5.0], [4.0, 4.0, 4.0, 4.0], [0.0, 1.0, 2.0, 9.0]])
    assert OB.argmax_lowest(q).tolist() == [1, 0, 0, 3]


@pytest.mark.parametrize("case", EC.losses(), ids=lambda c: c["name"])
def test_loss_tables_against_autograd(case):
    q = case["q"].clone().requires_grad_(True)
    val, prio = OB.loss(q, case["act"], case["ret"], case["weight"])
    (dq,) = torch.autograd.grad(val, q)
    want = EC.expected_dq(case["q"], case["act"], case["ret"], case["weight"])
    np.testing.assert_allclose(dq.numpy(), want.numpy(), rtol=1e-12, atol=1e-15)
    td = OB.td_errors(case["q"], case["act"], case["ret"])
    np.testing.assert_allclose(prio.detach().numpy(), td.sum(-1).numpy(), rtol=0, atol=0)
    # the dueling backward of q = v + adv - mean_a adv: dAdv sums to zero over a, dV is the sum of dQ
    d_adv = dq - dq.mean(-1, keepdim=True)
    assert float(d_adv.sum(-1).abs().max()) <= 1e-12 * max(float(dq.abs().max()), 1e-300) * dq.shape[-1]
    if case["name"] == "td_cancel_in_the_priority":
        assert prio.tolist() == [0.0, 0.0] and float(td.abs().max()) == 1000.0
    if case["weight"] is not None:
        assert not dq[case["weight"] == 0].any()


@pytest.mark.parametrize("kind", ["equal", "offset"])
def test_combine_edges(kind):
    dims = (5, (20,), 33, 20, 3, 5, "relu")
    p = EC.combine_params(dims, kind)
    obs = torch.randn(6, 5, generator=torch.Generator().manual_seed(2))
    q = OB.forward(p, dims, obs)
    v = OB.forward({k: (torch.zeros_like(t) if k.startswith("branches") else t) for k, t in p.items()}, dims, obs)[:, :1, :1]
    want = v.expand_as(q) if kind == "equal" else (v + (torch.arange(5.0) - 2.0)).expand_as(q)
    assert torch.equal(q, want)


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_dueling_invariants_in_float64(name):
    c = EC.shape_case(name)
    dims = c["dims"]
    params = {k: v.clone().requires_grad_(True) for k, v in c["params"].items()}
    pre: list = []
    q = OB.forward(params, dims, c["obs"], pre)
    q.retain_grad()
    val, _ = OB.loss(q, c["act"], c["ret"], c["weight"])
    val.backward()
    np.testing.assert_allclose(q.grad.numpy(), EC.expected_dq(q.detach(), c["act"], c["ret"], c["weight"]).numpy(), rtol=1e-12, atol=1e-18)
    # d loss / d (value head bias) = sum_b dV[b] = sum of dQ; d loss / d (branch head bias) sums to zero over a
    hv, ha = dims[2], dims[3]
    np.testing.assert_allclose(float(params[f"value.model.{2 if hv else 0}.bias"].grad), float(q.grad.sum()), rtol=1e-10, atol=1e-18)
    for d in range(dims[4]):
        gb = params[f"branches.{d}.model.{2 if ha else 0}.bias"].grad
        assert abs(float(gb.sum())) <= 1e-12 * max(float(gb.abs().max()), 1e-300) * dims[5]


def test_float32_oracle_stays_within_half_the_tolerances():
    worst = dict(q=0.0, grad=0.0, loss=0.0, prio=0.0)
    for name in SHAPE_NAMES:
        c = EC.shape_case(name)
        dims = c["dims"]
        out = {}
        for dt in (torch.float32, torch.float64):
            a = OB.Agent({k: v.to(dt) for k, v in c["params"].items()}, dims, gamma=0.99)
            g, val, prio = a.gradient(c["obs"].to(dt), c["act"], c["ret"].to(dt), c["weight"].to(dt))
            out[dt] = (a.q(c["obs"].to(dt)).double(), torch.cat([g[k].reshape(-1) for k in OB.state_keys(dims)]).double(), float(val), prio.double())
        (q32, g32, l32, p32), (q64, g64, l64, p64) = out[torch.float32], out[torch.float64]
        td = float(OB.td_errors(q64, c["act"], c["ret"]).abs().max())
        worst["q"] = max(worst["q"], float(((q32 - q64).abs() / (BC.RTOL * q64.abs() + BC.Q_ATOL)).max()))
        worst["grad"] = max(worst["grad"], float((g32 - g64).abs().max() / g64.abs().max()))
        worst["loss"] = max(worst["loss"], abs(l32 - l64) / abs(l64))
        worst["prio"] = max(worst["prio"], float((p32 - p64).abs().max()) / (td * dims[4]))
    print("float32 oracle against float64:", worst)
    assert worst["q"] <= 0.5 and worst["grad"] <= BC.GRAD_RTOL / 2 and worst["loss"] <= BC.RTOL / 2 and worst["prio"] <= 1e-5 / 2
