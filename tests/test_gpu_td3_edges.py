"""The deterministic head kernels of ts_sac.hip (det_policy_kernel, det_policy_bwd_kernel) at saturation and at the clip of TD3's
target-smoothing noise: head values of +-12 (tanh == +-1.0f), noise * policy_noise exactly on +-noise_clip, one float32 inside it
and far outside it, and noise_clip = 0 (no clamp).  Inputs: tests/sac_edge_cases.py::det_case (checked on the CPU by
tests/test_sac_edge_inputs_cpu.py).  policy_noise = 0.25 and noise_clip = 0.5 are powers of two, so the products are exact in
float32 and float64 and "exactly on the clip" means the same entry in both."""
import numpy as np
import pytest
import torch

from oracle import oracle_sac as OS
from tests import sac_edge_cases as E

pytestmark = pytest.mark.gpu
OBS, HID, MAX_ACTION = 7, 64, 1.5
CFG_KEYS = ("gamma", "tau", "n_step", "twin", "policy_noise", "noise_clip", "update_actor_freq", "max_action", "actor_lr", "critic_lr")


def engine_from(case, cfg):
    """tests/test_gpu_td3.py::make_engine with the case's parameters instead of freshly initialised ones."""
    from tianshou_amd import td3 as T
    from tianshou_amd import widths as W

    lists = [list(case["actor"].values()), list(case["critic1"].values())] + ([list(case["critic2"].values())] if cfg.twin else [])
    H = W.engine_hidden([W.layer_widths(t, 1) for t in lists])
    obs_dim, act_dim = case["obs"].shape[1], case["actor"]["ba"].numel()
    return T.TD3Engine(obs_dim, act_dim, T.actor_flat_from_torch(lists[0], obs_dim, act_dim, hidden=H),
                       T.critic_flat_from_torch(lists[1], obs_dim, act_dim, hidden=H),
                       T.critic_flat_from_torch(lists[2], obs_dim, act_dim, hidden=H) if cfg.twin else None,
                       T.TD3Config(**{k: getattr(cfg, k) for k in CFG_KEYS}), hidden=H, depth=OS.depth_of(case["actor"]))


def config(twin, noise_clip=E.TD3_NOISE_CLIP):
    return OS.TD3Config(twin=twin, max_action=MAX_ACTION, policy_noise=E.TD3_POLICY_NOISE, noise_clip=noise_clip, actor_lr=0.0,
                        critic_lr=0.0, tau=0.0, update_actor_freq=1)


@pytest.mark.parametrize("twin", [True, False])
@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("A", [1, 6, 32])
def test_deterministic_head_at_saturation_and_at_the_noise_clip(A, B, twin):
    """Saturated columns: the action is exactly +-max_action and the actor's gradient exactly 0 there (1 - tanh^2 == 0.0f); the free
    columns' gradient against float64 at the suite's 2e-5.  target_q with noise on / inside / beyond the clip, and with
    noise_clip = 0 (where the far-out entries of +-10 go straight into the critics), against the float64 oracle at 1e-5."""
    from tianshou_amd import td3 as T

    case = E.det_case(OBS, A, B, 4, twin, HID)
    cfg = config(twin)
    eng = engine_from(case, cfg)
    cols = case["cols"]
    act = eng.policy_forward(case["obs"]).cpu()
    act64 = OS.det_actor_forward(E.double(case["actor"]), case["obs"].double(), MAX_ACTION)
    for j in cols["saturated"]:
        assert bool((act[:, j] == MAX_ACTION * float(torch.sign(case["actor"]["ba"][j]))).all()), j
    np.testing.assert_allclose(act.numpy(), act64.numpy(), rtol=1e-6, atol=1e-6)
    tqs = {}
    for clip in (E.TD3_NOISE_CLIP, 0.0):
        e = eng if clip else engine_from(case, config(twin, clip))
        tq = tqs[clip] = e.target_q(case["obs"], case["noise"] if twin else None).cpu()
        tq64 = E.td3_target64(case, MAX_ACTION, E.TD3_POLICY_NOISE, clip, twin)
        assert torch.isfinite(tq).all()
        np.testing.assert_allclose(tq.numpy(), tq64.numpy(), rtol=1e-5, atol=1e-5, err_msg=f"noise_clip {clip}")
    if twin and B > 1:
        # the engine's clamp is live: its two targets differ (in float64 by more than 0.1, tests/test_sac_edge_inputs_cpu.py)
        assert float((tqs[E.TD3_NOISE_CLIP] - tqs[0.0]).abs().max()) > 0.1
    pc = eng.critic1.numel()
    grads = torch.zeros(2 * pc + eng.actor.numel(), dtype=torch.float32, device="cuda")
    stats, w = eng.update_with_batch(case["obs"], case["act"], case["ret"], grads_out=grads)
    assert torch.isfinite(grads).all() and torch.isfinite(stats).all() and torch.isfinite(w).all()
    sa, _ = OS.layer_sizes(HID)
    got = dict(zip(case["actor"].keys(), (t.cpu() for t in T.actor_flat_to_torch(grads[2 * pc:], OBS, A, eng.hidden, sizes=sa))))
    for j in cols["saturated"]:
        assert float(got["ba"][j]) == 0.0 and not got["wa"][j].any(), j
    p = {k: v.double().requires_grad_(True) for k, v in case["actor"].items()}
    loss = -OS.critic_forward(E.double(case["critic1"]), case["obs"].double(), OS.det_actor_forward(p, case["obs"].double(), MAX_ACTION)).mean()
    g64 = dict(zip(p, torch.autograd.grad(loss, list(p.values()))))
    np.testing.assert_allclose(float(stats[0]), float(loss), rtol=1e-5, atol=1e-6)
    if len(cols["free"]):
        for k in ("wa", "ba"):
            assert float(g64[k].abs().max()) > 0.0
            err = float((got[k].double() - g64[k]).abs().max() / g64[k].abs().max())
            assert err < 2e-5, (k, err)
