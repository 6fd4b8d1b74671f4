"""CPU: tests/oracle_icm_cnn.py reproduces the reference's two recorded runs (tests/golden/icm_cnn_*.npz): mse_loss, act_hat, the
augmented rewards, the three statistics, the parameters after both updates and the optimizer moments, in float32 as the
reference computed them (bars: the recorded-run bars of test_gpu_icm.py); the fixtures meet their own ReLU margin."""
import numpy as np
import pytest
import torch

from tests import icm_cnn_cases as CS
from tests import oracle_icm_cnn as OC


@pytest.mark.parametrize("tag", ["small", "odd"])
def test_oracle_reproduces_the_recorded_run(tag):
    g = CS.load(tag)
    c, stride = g["cfg"], g["d"]["stride"]
    assert g["relu_min_abs"].shape == g["relu_f32_err"].shape and g["relu_min_abs"].shape[0] == 2
    assert bool((g["relu_min_abs"] >= 64 * g["relu_f32_err"]).all())
    for dtype in (torch.float32, torch.float64):
        opt = OC.Optim(CS.fixture_model(g, dtype), "adam", lr=c["icm_lr"])
        for u in range(2):
            obs, act, nxt, rew = CS.fixture_rows(g, u)
            lo, err = OC.relu_margins(OC.cast(opt.model(), torch.float32), obs, act, nxt)
            if dtype == torch.float32:
                np.testing.assert_allclose(lo, g["relu_min_abs"][u], rtol=1e-3)           # the margin is the recorded one
            with torch.no_grad():
                mse, act_hat = OC.forward(opt.model(), obs, act, nxt)
            np.testing.assert_allclose(mse.numpy(), g[f"u{u}_pre_mse"], rtol=1e-5)
            np.testing.assert_allclose(act_hat.numpy().reshape(-1)[::stride], g[f"u{u}_pre_act_hat"], rtol=1e-5,
                                       atol=1e-5 * float(np.abs(g[f"u{u}_pre_act_hat"]).max()))
            np.testing.assert_allclose((OC.reward(rew, mse.float(), c["reward_scale"]) - rew).numpy(),
                                       g[f"u{u}_pre_rew_after"] - g[f"u{u}_pre_rew_before"], rtol=1e-5, atol=1e-12)
            stats = OC.update(opt, obs, act, nxt, c["forward_loss_weight"], c["lr_scale"])
            np.testing.assert_allclose(stats.numpy(), g[f"u{u}_icm_stats"], rtol=1e-5)
            np.testing.assert_allclose(CS.cat(opt.model())[::stride], g[f"u{u}_i"], rtol=1e-4, atol=0.02 * c["icm_lr"])
        state = opt.opt.state
        m = torch.cat([state[p]["exp_avg"].reshape(-1) for p in opt.params]).double().numpy()[::stride]
        v = torch.cat([state[p]["exp_avg_sq"].reshape(-1) for p in opt.params]).double().numpy()[::stride]
        np.testing.assert_allclose(m, g["adam_m_i"], rtol=1e-3, atol=max(1e-6, 2e-7 * float(np.abs(g["adam_m_i"]).max())))
        np.testing.assert_allclose(v, g["adam_v_i"], rtol=1e-3, atol=1e-8 * max(1.0, float(np.abs(g["adam_v_i"]).max())))
