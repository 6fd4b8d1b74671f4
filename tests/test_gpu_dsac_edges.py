"""DiscreteSAC's softmax / entropy kernels of ts_sac.hip on both routes -- 32 lanes per sample (dsac_target32_kernel,
dsac_actor32_kernel: n_act <= 32) and one thread per sample (dsac_target_kernel, dsac_actor_kernel) -- on rows a fresh network never
produces: one logit 40 or 120 above the rest (p e^-40, and p == 0.0f where p log p must be -0, not NaN), all logits equal
(H = log n_act), two tied maxima, Q1 == Q2 in every third column; and `spread`, whose rows differ, so that a lane reading its
neighbour's sample shows.  Inputs: tests/sac_edge_cases.py::dsac_case (checked on the CPU by tests/test_sac_edge_inputs_cpu.py).

Bar: within max(1e-5, 2 e_ref) of the float64 yardstick on each tensor's scale, e_ref being the float32 oracle's own distance.
Measured, largest over all cases (float32 oracle e_ref / engine on an MI355X): target 1.4e-05 / 1.4e-05 and actor loss 1.4e-05 /
1.4e-05 (n_act 2, all logits equal: alpha H and sum p q nearly cancel; 7e-07 elsewhere), mean neg_ent 2.6e-07 / 2.8e-07, head.b
gradient 1.7e-06 / 2.7e-06, head.w gradient 1.6e-06 / 2.8e-06.  Under a dominant logit the gradient is e^-40 of its terms and
the float32 oracle is 100 % off on the tensor's own scale (the engine 7 %): there an absolute criterion is asserted as well."""
import numpy as np
import pytest
import torch

from oracle import oracle_dsac as ODS
from oracle import oracle_sac as OS
from tests import sac_edge_cases as E

pytestmark = pytest.mark.gpu
OBS, HID, LOG_ALPHA = 7, 64, -0.3
CFG_KEYS = ("gamma", "tau", "n_step", "alpha", "auto_alpha", "target_entropy", "log_alpha0", "actor_lr", "critic_lr", "alpha_lr")


def engine_from(case, cfg):
    """tests/test_gpu_dsac.py::make_engine with the case's parameters instead of freshly initialised ones."""
    from tianshou_amd import dsac as DS
    from tianshou_amd import widths as W
    from tianshou_amd.sac import SACConfig

    nets = [case[k] for k in ("actor", "critic1", "critic2")]
    obs_dim, n_act = case["obs"].shape[1], case["actor"]["head.b"].numel()
    H = W.engine_hidden([W.layer_widths(list(p.values()), 1) for p in nets])
    flats = [DS.net_flat_from_torch(list(p.values()), obs_dim, n_act, H) for p in nets]
    return DS.DiscreteSACEngine(obs_dim, n_act, H, *flats, SACConfig(**{k: getattr(cfg, k) for k in CFG_KEYS}), depth=2)


def scale_err(x, exact):
    x, exact = torch.as_tensor(x).double(), torch.as_tensor(exact).double()
    return float((x - exact).abs().max() / exact.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("n_act", [2, 31, 32, 33, 64])
@pytest.mark.parametrize("pattern", E.DSAC_PATTERNS)
def test_softmax_and_entropy_at_dominance_equality_and_ties(pattern, n_act, B):
    """31 / 32 / 33 straddle the switch between the two routes (32: no dead lane); B = 257 leaves a half-wave pair whose second
    sample is out of range.  Target value, -H, actor loss and the logits-bias gradient of one update (learning rates 0)."""
    from tianshou_amd import dsac as DS

    case = E.dsac_case(OBS, n_act, B, 5, pattern, HID)
    cfg = OS.SACConfig(auto_alpha=True, log_alpha0=LOG_ALPHA, target_entropy=0.98 * float(np.log(n_act)), actor_lr=0.0,
                       critic_lr=0.0, alpha_lr=0.0, tau=0.0)
    eng = engine_from(case, cfg)
    st = OS.SACState.create(case["actor"], case["critic1"], case["critic2"], cfg)
    alpha = OS.alpha_value(st, cfg)
    y = E.dsac64(case, alpha)
    tq32 = ODS.target_q(st, cfg, case["obs"])
    col: dict = {}
    ref = ODS.update_with_batch(st, cfg, case["obs"], case["act"], case["ret"], collect=col)
    tq = eng.target_q(case["obs"]).cpu()
    P = eng.lay["count"]
    grads = torch.empty(3 * P, dtype=torch.float32, device="cuda")
    stats, w = eng.update_with_batch(case["obs"], case["act"], case["ret"], grads_out=grads)
    assert torch.isfinite(tq).all() and torch.isfinite(stats).all() and torch.isfinite(w).all() and torch.isfinite(grads).all()
    got = dict(zip(ODS.NET_ORDER, (t.cpu() for t in DS.net_flat_to_torch(grads[2 * P:], OBS, n_act, HID))))
    # neg_ent is workspace memory with no per-row output.  Per row, H is carried by the target value f = alpha H + sum p q below;
    # the alpha loss -(log_alpha * (target_entropy + neg_ent)).mean() adds the batch mean of neg_ent as the actor step computed
    # it, measured against log_alpha * (target_entropy + H) -- an error that cancels in the mean would show only in f
    al64 = -LOG_ALPHA * (cfg.target_entropy + float(y["neg_ent"].mean()))
    al_scale = abs(LOG_ALPHA) * (cfg.target_entropy + float(-y["neg_ent"].mean()))
    e_gpu, e_ref = abs(float(stats[4]) - al64) / al_scale, abs(ref["alpha_loss"] - al64) / al_scale
    print(f"n_act={n_act} B={B} {pattern}: mean neg_ent (alpha loss) engine {e_gpu:.2e} float32 oracle {e_ref:.2e}")
    assert e_gpu < max(1e-5, 2 * e_ref), (pattern, "neg_ent", e_gpu, e_ref)
    q_max = float(torch.max(case["critic1"]["head.b"].abs().max(), case["critic2"]["head.b"].abs().max()))
    terms = q_max + alpha * float(np.log(n_act))
    hmax = float(E.dsac_hidden(case).abs().max())
    checks = [("target", tq, tq32, y["target"]), ("actor_loss", stats[0], ref["actor_loss"], y["actor_loss"]),
              ("head.b gradient", got["head.b"], col["actor_grads"]["head.b"], y["actor_grads"]["head.b"]),
              ("head.w gradient", got["head.w"], col["actor_grads"]["head.w"], y["actor_grads"]["head.w"])]
    for name, x, x32, exact in checks:
        if float(torch.as_tensor(exact).abs().max()) == 0.0:
            assert not torch.as_tensor(x).any(), (pattern, name)
            continue
        e_gpu, e_ref = scale_err(x, exact), scale_err(x32, exact)
        print(f"n_act={n_act} B={B} {pattern}: {name} engine {e_gpu:.2e} float32 oracle {e_ref:.2e}")
        assert e_gpu < max(1e-5, 2 * e_ref), (pattern, name, e_gpu, e_ref)
        # where a dominant logit leaves a gradient of e^-40 of its terms the float32 oracle is 100 % off on the tensor's own
        # scale and the bar above says nothing: the error must also be small against the terms
        # p (q - sum p q) - alpha p (log p + H)
        if name.endswith("gradient"):
            term_scale = terms * (hmax if name.startswith("head.w") else 1.0)
            abs_err = float((torch.as_tensor(x).double() - exact).abs().max())
            assert abs_err <= 1e-5 * max(float(exact.abs().max()), term_scale), (pattern, name, abs_err)
    if pattern == "equal":
        H = cfg.target_entropy + float(stats[4]) / LOG_ALPHA                           # mean entropy, from the alpha loss
        assert abs(H - np.log(n_act)) <= 1e-6 * max(1.0, float(np.log(n_act))), (H, np.log(n_act))
