"""The Categorical PPO / A2C loss kernels at their clip, tie and logit edges, one homogeneous batch per edge
(tests/ppo_edge_cases.py states the construction, the float64 references and the bar):

  copy 5   ts_ppo_cnn.hip cnn_ppo_loss_kernel (per-step path)           DiscretePPOEngine.step(grad_out=, apply=False)
  copy 6   ts_mlp_small.hip (the whole update in one launch)            DiscretePPOEngine.update
  copy 7   the A2C branch of both: the "ratio_a2c" group and the a2c cases of "logits"

CnnPPOEngine launches copy 5's kernel and needs 84 x 84 inputs: it is left out.  Copy 6 exposes only losses and post-Adam
parameters: its step-1 losses are held to the float64 bar, and the loss rows and final parameters of a 3-step update on the edge
batches to the per-step path (TS_MLP_PPO_PER_STEP=1) at the tolerances tests/test_gpu_ppo_discrete.py uses for that comparison.

Logits: all equal (p = 1 / A exactly), one dominating by 20, 90 (exp underflows to a subnormal) and 1e4 (to zero), graded;
A = 1 (logp = 0, entropy, logit and actor gradients exactly 0), 2, 18, 31; act on the dominant and on a dominated column.  The
head block's padding columns j > A are exactly 0.

Measured on an MI355X, worst |gpu - ref64| / (eps32 * scale) over all cases:
                                   losses   logit bias  logit weight  V bias  V weight
  copy 5  ratio / advnorm / value   5.2      10.6        14.2          0.4     2.5
          logits                    4.6       6.3         5.3          0.3     2.0
  copy 6  step-1 losses             5.7   (ratio groups; 5.0 on logits, 1.2 on the others)
The float32 oracle's own figures on the same cases: 5.2 / 10.6 / 14.5 / 0.4 / 1.4.

Found by test_copy6_one_launch_update[logits_dom1e4] and fixed in ts_mlp_small.hip: the one-launch kernel started its head
accumulator at the bias, so with a logit of 1e4 (float32 spacing 9.8e-4) every partial sum was rounded at that spacing.  Step 1
(zero head weights) agreed with float64 and with the per-step path bit for bit; from step 2 on, with head weights of +-lr, its
clip losses were up to 3.9e-3 off the per-step path's (case A2 / dom10000 / act_cold / dual_off / B33: -1.651657 against
-1.654843, -1.676282 against -1.678834) where the comparison allows 5e-5 -- a float32 emulation of "bias first" against "bias
last" on that case puts the two logits up to 7 spacings apart, the first 6.4e-3 and the second 4.7e-4 from float64.  The kernel
now adds the bias last, to the finished sum, as the GEMM path (ts_conv.hip) does; its outputs change in the last bits on ordinary
inputs (one rounding at the bias's size instead of 64)."""
import numpy as np
import pytest
import torch

from oracle import oracle_ppo_discrete as OD
from tests import ppo_edge_cases as E

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
GROUPS = ["ratio_dual_off", "ratio_dual_on", "ratio_a2c", "advnorm", "value", "logits", "logits_dom1e4"]
OBS_DIM, HIDDEN, _ = E.KINDS["discrete"]


def make_engine(case, r):
    from tianshou_amd import ppo as P
    from tianshou_amd import ppo_discrete as PD

    A = len(case["head"]["logits"])
    flat = PD.flat_from_torch([r["params"][k] for k in OD.PARAM_ORDER], OBS_DIM, HIDDEN, A)
    return A, PD.DiscretePPOEngine(OBS_DIM, HIDDEN, A, flat, P.PPOConfig(**case["hp"]))


@pytest.mark.parametrize("group", GROUPS)
def test_copy5_per_step_loss_kernel(group):
    from tianshou_amd import ppo_discrete as PD

    worst: dict = {}
    cases = E.cat_cases(group)
    for case in cases:
        r = E.reference("discrete", case)
        A, eng = make_engine(case, r)
        rows = case["rows"]
        grad = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
        losses = eng.step(r["obs"], rows["act"], rows["adv"], rows["returns"], rows["logp_old"], rows["v_s"], grad_out=grad, apply=False)
        torch.cuda.synchronize()
        named = dict(zip(OD.PARAM_ORDER, PD.flat_to_torch(grad, OBS_DIM, HIDDEN, A)))
        what = f"copy5 {case['name']}"
        E.check(losses.double().cpu().numpy(), {k: named[k].double().cpu().numpy() for k in r["blocks"]}, r, worst, what)
        for k in r["trunk"]:
            assert not bool(named[k].any()), (what, k)
        for k in E.exact_zero_blocks("discrete", case):
            assert not bool(named[k].any()), (what, k, "must be exactly zero")
        lay = PD.layout(OBS_DIM, HIDDEN, A)
        head = grad[-(HIDDEN + 1) * lay["head"]:].reshape(HIDDEN + 1, lay["head"])
        assert not bool(head[:, A + 1:].any()), (what, "padding columns")          # (column A is the critic's)
        assert torch.isfinite(grad).all(), what
    print(f"\n  copy5 {group}: {len(cases)} cases, worst |gpu - ref64| / (eps32 * scale): " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))


def _update(case, r, repeat, monkeypatch, per_step):
    from tianshou_amd.buffer import DeviceReplayBuffer

    if per_step:
        monkeypatch.setenv("TS_MLP_PPO_PER_STEP", "1")
    else:
        monkeypatch.delenv("TS_MLP_PPO_PER_STEP", raising=False)
    rows = case["rows"]
    n = len(rows["adv"])
    _, eng = make_engine(case, r)
    buf = DeviceReplayBuffer.from_vector_fill(1, rew=np.zeros(n), terminated=np.zeros(n, bool), truncated=np.zeros(n, bool), obs=r["obs"],
                                              act=rows["act"], obs_next=r["obs"])
    pre = {k: torch.as_tensor(rows[k]).cuda() for k in ("adv", "returns", "logp_old", "v_s")}
    pre["indices"] = torch.arange(n, device="cuda")
    pre["act"] = torch.as_tensor(rows["act"]).cuda()
    losses, steps = eng.update(buf, pre, n, repeat, [np.arange(n) for _ in range(repeat)])
    torch.cuda.synchronize()
    assert steps == repeat == eng.adam_step
    return losses.double().cpu().numpy(), eng.params.cpu().numpy()


@pytest.mark.parametrize("group", GROUPS)
def test_copy6_one_launch_update(group, monkeypatch):
    from tianshou_amd import _lib

    worst: dict = {}
    cases = E.cat_cases(group)
    assert _lib.load().ts_mlp_ppo_update_supported(_lib.i64(OBS_DIM), _lib.i64(HIDDEN), _lib.i64(31))
    for case in cases:
        r = E.reference("discrete", case)
        what = f"copy6 {case['name']}"
        one, p_one = _update(case, r, 3, monkeypatch, per_step=False)
        per, p_per = _update(case, r, 3, monkeypatch, per_step=True)
        # step 1 runs on the edge network itself: float64 under the bar
        diff = np.abs(one[0] - r["losses"])
        s = r["scales"]["losses"]
        worst["losses"] = max(worst.get("losses", 0.0), float((np.maximum(diff - r["floor"], 0.0) / np.where(s > 0, E.EPS32 * s, 1.0)).max()))
        assert np.all(np.isfinite(one)) and np.all(diff <= r["bars"]["losses"]), (what, one[0], r["losses"], r["bars"]["losses"])
        # ... and three steps against the per-step path (tests/test_gpu_ppo_discrete.py's tolerances for this comparison)
        np.testing.assert_allclose(one, per, rtol=5e-5, atol=2e-6, err_msg=what)
        np.testing.assert_allclose(p_one, p_per, rtol=1e-5, atol=0.05 * case["hp"]["lr"], err_msg=what)
    print(f"\n  copy6 {group}: {len(cases)} cases, worst step-1 |loss - ref64| / (eps32 * scale): {worst['losses']:.2f}")
