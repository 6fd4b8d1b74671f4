"""The TD3+BC kernels of ts_sac.hip (td3bc_actor_loss_kernel, td3bc_policy_bwd_kernel) against float64 autograd of the oracle
formula (tests/oracle_td3bc.py::actor_loss_terms) at their edges: Q of both signs whose mean cancels, Q negative everywhere,
saturated head columns, actions cloned bit for bit, alpha = 0.  A in {1, 6, 32} x B in {1, 257, 1025}: one column, a partly
filled row and all 32 head columns; one row, one past the 256 threads of the backward kernel's workgroup and one past the 1024
of the loss kernel's (so its workgroup 0 loops and a third workgroup writes d_q), none a multiple of the 64-lane wavefront.
Inputs: tests/td3bc_edge_cases.py (checked on the CPU by tests/test_td3bc_edge_inputs_cpu.py: mean|Q| >= 0.05 in every case, so
nothing is excluded here).  Tolerances are tests/test_gpu_td3_edges.py's: loss rtol 1e-5 / atol 1e-6, gradients 2e-5 of the
tensor's largest entry; lmbda at rtol 1e-5."""
import numpy as np
import pytest
import torch

from oracle import oracle_sac as OS
from tests import oracle_td3bc as OB
from tests import td3bc_common as CC
from tests import td3bc_edge_cases as E

pytestmark = pytest.mark.gpu
OBS, HID = 7, 64


def run(case):
    """One gradient-only update (actor_lr = critic_lr = -1, tau = 0) -> (stats [4], the actor's gradient by oracle name)."""
    from tianshou_amd import td3 as T

    cfg = OB.TD3BCConfig(max_action=E.MAX_ACTION, actor_lr=-1.0, critic_lr=-1.0, tau=0.0, update_actor_freq=1, alpha=case["alpha"])
    eng = CC.engine_from(case["actor"], case["critic1"], case["critic2"], cfg)
    pc = eng.critic1.numel()
    grads = torch.zeros(2 * pc + eng.actor.numel(), dtype=torch.float32, device="cuda")
    stats, w = eng.update_with_batch(case["obs"], case["act"], case["ret"], grads_out=grads)
    assert torch.isfinite(grads).all() and torch.isfinite(stats).all() and torch.isfinite(w).all()
    A = case["actor"]["ba"].numel()
    sa, _ = OS.layer_sizes(HID)
    got = dict(zip(case["actor"].keys(), (t.cpu() for t in T.actor_flat_to_torch(grads[2 * pc:], OBS, A, eng.hidden, sizes=sa))))
    return stats.cpu(), got


def close(got, want, keys, what):
    for k in keys:
        scale = float(want[k].abs().max())
        assert scale > 0.0, (what, k)
        err = float((got[k].double() - want[k]).abs().max()) / scale
        assert err < 2e-5, (what, k, err)


@pytest.mark.parametrize("B", [1, 257, 1025])
@pytest.mark.parametrize("A", [1, 6, 32])
@pytest.mark.parametrize("kind", E.KINDS)
def test_td3bc_actor_kernels_at_their_edges(kind, A, B):
    case = E.edge_case(kind, OBS, A, B, 4, HID)
    ref = E.reference64(case)
    stats, got = run(case)
    cols = case["cols"]
    lmbda, loss = float(stats[3]), float(stats[0])
    if kind == "alpha0":
        assert lmbda == 0.0                                                     # exactly: 0 / mean|Q|
        np.testing.assert_allclose(loss, ref["bc_loss"], rtol=1e-5, atol=1e-6)
        close(got, ref["bc"], ("wa", "ba") + (("w1", "b1", "w2", "b2")), "mse_loss alone")
        return
    assert lmbda > 0.0                                                          # also where every Q < 0
    np.testing.assert_allclose(lmbda, ref["lmbda"], rtol=1e-5)
    np.testing.assert_allclose(loss, ref["loss"], rtol=1e-5, atol=1e-6)
    for j in cols["saturated"]:                                                 # 1 - tanh^2 == 0.0f
        assert float(got["ba"][j]) == 0.0 and not got["wa"][j].any(), j
    if len(cols["free"]):
        close(got, ref["grads"], ("wa", "ba"), "head")
    if kind in ("mixed", "negative"):
        close(got, ref["grads"], ("w1", "b1", "w2", "b2"), "trunk")
    if kind == "cloned":
        np.testing.assert_allclose(loss, -ref["lmbda"] * float(ref["q"].mean()), rtol=1e-5, atol=1e-6)
        close(got, {k: ref["lmbda"] * v for k, v in ref["td3"].items()}, ("wa", "ba"), "lmbda x plain TD3")
