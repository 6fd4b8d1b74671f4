"""The fused cosine-embedding kernels of ts_iqn.hip (iqn_embed_fwd_kernel<2>, iqn_embed_bwd_kernel) where their row-tile loops
run more than once per workgroup, and the route every entry point takes from 2^14 rows on -- alone, at the route boundary, and
inside the engine (`update_with_batch` at R = 16448, `forward` at the evaluation shape R = 512 * 32).

Yardstick: float64, with the cosine arguments formed in float32 as the reference forms them (tests/iqn_edge_cases.py).  Bar of
every tensor: max(1e-5, 2 e_ref) of its scale -- 1e-5 is the project's own bar (tests/test_gpu_iqn.py), e_ref the float32 torch
expression's own rel_err against float64 on the same input (sums over 16384 rows may legitimately exceed 1e-5); it is computed
from the reference alone and printed.  tests/test_iqn_edge_inputs_cpu.py recomputes the tile and share counts of every shape."""
import numpy as np
import pytest
import torch

from tests import iqn_edge_cases as E
from tests import oracle_iqn as OI
from tests.distq_edge_gpu_common import SENTINEL, dev_obs

pytestmark = pytest.mark.gpu


def check(got, ref, e_ref, what):
    """rel_err(got, ref64) < max(1e-5, 2 e_ref); prints the figures and the ratio to the bar."""
    e, bar = E.rel_err(got.cpu() if isinstance(got, torch.Tensor) else got, ref), E.rel_bar(e_ref)
    print(f"    {what}: engine {e:.2e}, float32 reference {e_ref:.2e}, bar {bar:.2e}, engine / bar = {e / bar:.3f}")
    assert np.isfinite(e) and e < bar, (what, e, e_ref)


def embed_fwd(d, route):
    from tianshou_amd import iqn as I

    out = torch.full((d["tau"].numel(), d["feat"].shape[1]), SENTINEL, dtype=torch.float32, device="cuda")
    return I.embed_mul(d["tau"].cuda(), d["feat"].cuda(), d["we_be"].cuda(), out=out, route=route)


def embed_bwd(d, route):
    from tianshou_amd import iqn as I

    out = (torch.full(tuple(d["feat"].shape), SENTINEL, device="cuda"), torch.full(tuple(d["we_be"].shape), SENTINEL, device="cuda"))
    return I.embed_mul_backward(d["tau"].cuda(), d["feat"].cuda(), d["we_be"].cuda(), d["dx"].cuda(), out=out, route=route)


def check_bwd(shape, got, tag):
    ref = E.embed_reference(*shape, True)
    dfeat, dwe = got
    check(dfeat, ref["dfeat"], ref["e_dfeat"], f"{tag} dfeat")
    check(dwe[:64], ref["dwe"], ref["e_dwe"], f"{tag} dWe")
    check(dwe[64], ref["dbe"], ref["e_dbe"], f"{tag} dbe")


@pytest.mark.parametrize("B,N,F", E.FWD_SHAPES)
def test_fused_forward_with_several_tiles_per_share(B, N, F):
    """(157, 7, .): 18 row tiles over 16 shares with a partial last tile of 11 rows; F = 64 and 192 leave half of the last
    128-column tile outside F; tau = 0 and tau one ulp below 1 sit in the last tile."""
    d, ref = E.embed_inputs(B, N, F, False), E.embed_reference(B, N, F, False)
    tiles, shares = E.fwd_tiles(B, N)
    assert tiles > shares
    x = embed_fwd(d, "fused")
    print(f"  fused forward {(B, N, F)}: {tiles} tiles over {shares} shares")
    check(x, ref["x"], ref["e_x"], "x")
    assert torch.equal(x, embed_fwd(d, "fused"))
    if B * N < E.FUSED_FROM_ROWS:                                                     # the other route meets the same yardstick
        check(embed_fwd(d, "unfused"), ref["x"], ref["e_x"], "x (unfused)")


@pytest.mark.parametrize("B,N,F", E.BWD_SHAPES)
def test_fused_backward_with_several_tiles_per_share(B, N, F):
    """(157, 7): 18 tiles of 9 samples over 8 shares with a last tile of 4 samples; (19, 33): one half-empty tile per sample;
    (20, 64): one full tile per sample; (600, 1): 64 samples per tile.  Fractions are drawn off the ReLU kink."""
    d = E.embed_inputs(B, N, F, True)
    tiles, shares, sb = E.bwd_tiles(B, N)
    assert tiles > shares
    got = embed_bwd(d, "fused")
    print(f"  fused backward {(B, N, F)}: {tiles} tiles of {sb} samples over {shares} shares")
    check_bwd((B, N, F), got, "fused")
    again = embed_bwd(d, "fused")
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])            # bit-identical reruns
    check_bwd((B, N, F), embed_bwd(d, "unfused"), "unfused")


@pytest.mark.parametrize("shape,same_as", [(E.BOUNDARY_FUSED, "fused"), (E.BOUNDARY_UNFUSED, "unfused")])
def test_route_boundary(shape, same_as):
    """R = 16384: the default route IS the fused one, bit for bit, forward and backward; R = 16383: the unfused one."""
    assert (shape[0] * shape[1] >= E.FUSED_FROM_ROWS) == (same_as == "fused")
    d, ref = E.embed_inputs(*shape, False), E.embed_reference(*shape, False)
    x = embed_fwd(d, "default")
    assert torch.equal(x, embed_fwd(d, same_as))
    print(f"  route boundary {shape}: default == {same_as}")
    check(x, ref["x"], ref["e_x"], "x")
    d = E.embed_inputs(*shape, True)
    got, other = embed_bwd(d, "default"), embed_bwd(d, same_as)
    assert torch.equal(got[0], other[0]) and torch.equal(got[1], other[1])
    check_bwd(shape, got, "default")
    if same_as == "unfused":                                                          # one row below the boundary both exist
        check_bwd(shape, embed_bwd(d, "fused"), "fused")


def _engine(c):
    from tianshou_amd import iqn as I

    p, s = c["p"], c["tau"].shape
    A = p["fc2.b"].numel()
    eng = I.IQNEngine(E.C, E.H, E.W, A, I.flat_from_torch([p[k] for k in OI.PARAM_ORDER], E.C, E.H, E.W, A),
                      I.IQNConfig(online_sample_size=s[1], sample_size=s[1]))
    lay = I.layout(E.C, E.H, E.W, A)
    assert lay["F"] == E.FEAT and np.array_equal(lay["off"], E.layout_offsets(A))
    return eng, A


def test_engine_update_on_the_fused_default_route():
    """B = 257, N = 64, N' = 2 (R = 16448): loss, priorities and the gradient layer by layer against the float64 restatement of
    oracle_iqn.loss_terms; head padding exactly 0; bit-identical reruns."""
    c = E.engine_update_case()
    eng, A = _engine(c)
    assert c["tau"].numel() >= E.FUSED_FROM_ROWS
    runs = []
    for _ in range(2):
        grad = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
        loss, prio = eng.update_with_batch(dev_obs(c["obs"]), c["act"], c["ret"], c["weight"], tau=c["tau"].cuda(), grad_out=grad,
                                           apply=False)
        torch.cuda.synchronize()
        runs.append((loss.cpu(), prio.cpu(), grad.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    loss, prio, g = runs[0]
    print("  engine update at R = 16448")
    check(loss, c["loss"], c["e_ref"]["loss"], "loss")
    check(prio, c["prio"], c["e_ref"]["prio"], "prio")
    for k, (lo, hi) in c["parts"].items():
        check(g[lo:hi], c["grad"][lo:hi], c["e_ref"][k], f"gradient {k}")
    ld = E.head_ld(A)
    assert not g[-513 * ld:].reshape(513, ld)[:, A:].any()                            # head padding: exact zeros


def test_engine_forward_on_the_fused_default_route():
    """`forward` at B = 512, N = 32 (R = 16384 exactly, the evaluation shape over 512 environments): logits and Q within the bar,
    the action equal wherever the float64 gap to the runner-up is beyond float32 blur (at most 1 % of the rows are left out: a
    condition on the inputs that tests/test_iqn_edge_inputs_cpu.py asserts from the reference alone)."""
    c = E.engine_forward_case()
    eng, A = _engine(c)
    assert c["tau"].numel() == E.FUSED_FROM_ROWS
    for as_u8 in (True, False):
        x = dev_obs(c["obs"])
        lg, q, act = (t.cpu() for t in eng.forward(x if as_u8 else x.float(), tau=c["tau"].cuda()))
        print(f"  engine forward at R = 16384, uint8 observations: {as_u8}")
        check(lg, c["logits"], c["e_ref"]["logits"], "logits")
        check(q, c["q"], c["e_ref"]["q"], "q")
        clear = c["clear"]
        assert float(clear.double().mean()) >= 0.99
        assert torch.equal(act[clear], c["act"][clear])
        assert torch.equal(act, q.argmax(dim=1))
