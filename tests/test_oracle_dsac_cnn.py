"""CPU: tests/oracle_dsac_cnn.py -- the torch restatement of DiscreteSAC on the Atari trunk with three optimizers over a shared
trunk -- replays the recorded runs of the unmodified reference (tests/golden/dsac_cnn_*.npz, tools/gen_golden_dsac_cnn.py), and
its float32 deviation from a float64 run of itself is what tests/dsac_cnn_common.py records as the basis of the tolerances."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import dsac_cnn_common as DC
from tests import oracle_dsac_cnn as OS


def _cat(tensors) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1) for t in tensors]).double().numpy()


def replay(tag: str, dtype=torch.float32, fixture_returns: bool = False):
    """The fixture's update sequence through the oracle in `dtype` -> one dict per update and the final state."""
    g, d, cfg, bstate = DC.load(tag)
    p = {k: v.to(dtype) for k, v in OS.init_params(d["c"], d["h"], d["w"], d["n_act"], d["hidden"], d["seed"]).items()}
    st = OS.make_state(p, cfg)
    out = []
    for u in range(d["n_updates"]):
        idx = g[f"u{u}_indices"]
        ret, _ = O.compute_nstep_return(bstate, idx, lambda after: OS.target_q(st, cfg, g["frames_next"][after]).float().numpy(),
                                        cfg.gamma, cfg.n_step)
        ret = np.asarray(ret).reshape(-1)
        use = g[f"u{u}_returns"] if fixture_returns else ret
        stats, w = OS.update_with_batch(st, cfg, g["frames"][idx], g["act"][idx], use, DC.is_weight(g, d, u))
        out.append({"returns": ret, "stats": np.array([stats[k] for k in OS.STAT_NAMES]), "weight_out": w.double().numpy(),
                    "params": _cat([st.params[k] for k in OS.PARAM_ORDER]),
                    "biases": _cat([st.params[k] for k in OS.PARAM_ORDER if k.endswith(".b")]),
                    "lagged": _cat([st.params_old[k] for k in OS.LAGGED_ORDER]),
                    "log_alpha": float(st.log_alpha.detach())})
    return g, d, cfg, st, out


@pytest.mark.parametrize("tag", DC.TAGS)
def test_oracle_replays_reference_golden(tag):
    g, d, cfg, st, out = replay(tag)
    lr = DC.lr_of(cfg)
    n_t = sum(st.params[k].numel() for k in OS.TRUNK)
    for u, r in enumerate(out):
        np.testing.assert_allclose(r["returns"], g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
        DC.check_stats(r["stats"], g, u, cfg, d["n_act"])
        DC.check_weight(r["weight_out"], g, u)
        DC.check_params(r["params"][::DC.STRIDE], g[f"u{u}_params_strided"], DC.PARAM_DEV[tag][u], lr, f"{tag} u{u} parameters")
        DC.check_params(r["biases"], g[f"u{u}_biases"], DC.PARAM_DEV[tag][u], lr, f"{tag} u{u} biases")
        hd = (d["hidden"] + 1) * d["n_act"]
        lag = r["lagged"]
        for name, head in (("critic_old", lag[n_t:n_t + hd]), ("critic2_old", lag[n_t + hd:])):      # each: the ONE trunk + own head
            DC.check_params(np.concatenate([lag[:n_t], head])[::DC.STRIDE], g[f"u{u}_{name}_strided"], DC.LAGGED_DEV[tag][u], lr,
                            f"{tag} u{u} {name}")
        if cfg.auto_alpha:
            np.testing.assert_allclose(r["log_alpha"], float(g[f"u{u}_log_alpha"]), rtol=1e-5, atol=max(2 * DC.LOG_ALPHA_DEV[tag], 1e-7))
    for which in OS.SETS:
        m = _cat(list(st.moments(which, "exp_avg").values()))[::DC.STRIDE]
        v = _cat(list(st.moments(which, "exp_avg_sq").values()))[::DC.STRIDE]
        DC.check_moments(m, v, g, tag, which)
    # three DISTINCT trunk moment sets: the fixture's and the oracle's
    b = [g[f"adam_{s}_trunk_bias_m"] for s in OS.SETS]
    assert not np.allclose(b[0], b[1], rtol=1e-3) and not np.allclose(b[0], b[2], rtol=1e-3)
    if cfg.auto_alpha:
        s = st.alpha_opt.state[st.log_alpha]
        DC.check_alpha_moments(float(s["exp_avg"]), float(s["exp_avg_sq"]), g)
        assert float(s["step"]) == float(g["alpha_adam"][2])


@pytest.mark.parametrize("tag", DC.TAGS)
def test_float32_oracle_vs_float64(tag):
    """Measures what tests/dsac_cnn_common.py records: the float32 oracle against the float64 oracle on the fixture, both fed
    the fixture's returns so that the comparison is update by update.  Fails when a measurement exceeds its record."""
    g, d, cfg, st32, o32 = replay(tag, torch.float32, fixture_returns=True)
    _, _, _, st64, o64 = replay(tag, torch.float64, fixture_returns=True)
    lr = DC.lr_of(cfg)
    for u, (a, b) in enumerate(zip(o32, o64)):
        dev = float((np.abs(a["params"] - b["params"]) - DC.RTOL * np.abs(b["params"])).max() / lr)
        lag = float((np.abs(a["lagged"] - b["lagged"]) - DC.RTOL * np.abs(b["lagged"])).max() / lr)
        rel = float((np.abs(a["stats"][:4] - b["stats"][:4]) / np.abs(b["stats"][:4])).max())
        al = max(abs(a["stats"][4] - b["stats"][4]) - DC.RTOL * abs(b["stats"][4]), 0.0)
        dla = abs(a["log_alpha"] - b["log_alpha"])
        print(f"{tag} u{u}: params {dev:.3g} lr, lagged {lag:.3g} lr, stats {rel:.3g}, alpha_loss {al:.3g} beyond rtol, log_alpha {dla:.3g}")
        assert dev <= max(DC.PARAM_DEV[tag][u], 0.0) + 1e-12 or dev <= DC.ATOL_LR / DC.FACTOR
        assert lag <= max(DC.LAGGED_DEV[tag][u], 0.0) + 1e-12 or lag <= DC.ATOL_LR / DC.FACTOR
        assert rel <= max(DC.STAT_DEV[tag], DC.RTOL / DC.FACTOR)
        assert al <= max(DC.ALPHA_LOSS_DEV[tag], DC.ALPHA_LOSS_ATOL / DC.FACTOR)
        assert dla <= max(DC.LOG_ALPHA_DEV[tag], 5e-8)
    for which in OS.SETS:
        dev = []
        for kind in ("exp_avg", "exp_avg_sq"):
            x, y = _cat(list(st32.moments(which, kind).values())), _cat(list(st64.moments(which, kind).values()))
            dev.append(float(np.abs(x - y).max() / np.abs(y).max()))
        print(f"{tag} {which} moments: m {dev[0]:.3g}, v {dev[1]:.3g}")
        rec = DC.MOMENT_DEV[tag][which]
        assert dev[0] <= max(rec[0], 1e-5 / DC.FACTOR) and dev[1] <= max(rec[1], 2e-5 / DC.FACTOR)
    if cfg.auto_alpha:
        s32, s64 = st32.alpha_opt.state[st32.log_alpha], st64.alpha_opt.state[st64.log_alpha]
        dev = [abs(float(s32[k]) - float(s64[k])) / abs(float(s64[k])) for k in ("exp_avg", "exp_avg_sq")]
        print(f"{tag} log alpha moments: m {dev[0]:.3g}, v {dev[1]:.3g}")
        rec = DC.ALPHA_MOMENT_DEV[tag]
        assert dev[0] <= max(rec[0], 1e-5 / DC.FACTOR) and dev[1] <= max(rec[1], 2e-5 / DC.FACTOR)
