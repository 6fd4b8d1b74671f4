"""CPU: tests/oracle_cql.py (the torch restatement the GPU parity tests compare against) replays the fixtures recorded from
the UNMODIFIED reference CQL.update() on the CPU (tools/gen_golden_cql.py) at tests/test_oracle_td3bc.py's bars; where the
reference is mounted, the generator reproduces both files bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle_sac as OS
from oracle import ref_shim
from tests import cql_common as CC
from tests import oracle_cql as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", CC.TAGS)
def test_cql_restatement_matches_reference(tag):
    """Statistics rtol 1e-5 / atol 1e-7, networks rtol 1e-5 / atol 1e-6, first moments rtol 1e-5 / atol 1e-8, second moments
    rtol 1e-5 / atol 1e-12 (test_td3bc_restatement_matches_reference's bars); the critics' gradient norms before clipping and
    cql_log_alpha at the statistics' bar."""
    g, d, cfg = CC.load_cql(tag)
    st = OC.CQLState.create(*OS.init_sac_params(d["obs_dim"], d["act_dim"], d["seed"], d["hidden"]), cfg)
    with OS.activation(d["activation"]):
        for u in range(d["n_updates"]):
            out = OC.update_with_batch(st, cfg, **CC.batch_of(g, u, cfg.calibrated))
            np.testing.assert_allclose(CC.stats_vector(out), g[f"u{u}_stats"], rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose([out["critic1_grad_norm"], out["critic2_grad_norm"]], g[f"u{u}_grad_norms"], rtol=1e-5)
            np.testing.assert_allclose(float(st.cql_log_alpha), float(g[f"u{u}_cql_log_alpha"][0]), rtol=1e-5, atol=1e-7)
            for name in CC.NETS:
                p = getattr(st.sac, name)
                np.testing.assert_allclose(OS.flatten(p, OS.order_of(p)).numpy()[::61], g[f"u{u}_{name}"], rtol=1e-5, atol=1e-6,
                                           err_msg=name)
    for name, opt in (("actor", st.sac.opt_actor), ("critic1", st.sac.opt_c1), ("critic2", st.sac.opt_c2)):
        assert opt.step == int(g[f"adam_step_{name}"]) == d["n_updates"], name
        order = OS.order_of(getattr(st.sac, name))
        np.testing.assert_allclose(OS.flatten(opt.m, order).numpy()[::61], g[f"adam_m_{name}"], rtol=1e-5, atol=1e-8, err_msg=name)
        np.testing.assert_allclose(OS.flatten(opt.v, order).numpy()[::61], g[f"adam_v_{name}"], rtol=1e-5, atol=1e-12, err_msg=name)
    if cfg.with_lagrange:
        o = st.opt_cql_alpha
        np.testing.assert_allclose([o.step, float(o.m["a"]), float(o.v["a"])], g["adam_cql_alpha"], rtol=1e-5, atol=1e-12)


def test_fixtures_are_the_two_the_issue_describes():
    g, d, cfg = CC.load_cql("calibrated")
    assert d["hidden"] == ((256, 256), (256, 256)) and d["activation"] == "relu" and d["R"] == cfg.num_repeat_actions == 10
    assert cfg.auto_alpha and cfg.with_lagrange and cfg.calibrated and (d["min_action"], d["max_action"]) == (-1.0, 1.0)
    assert all(np.all(g[f"u{u}_random_act"] == 1.0) for u in range(d["n_updates"]))        # uniform_(1, 1)
    assert g["calibration_returns"].dtype == np.float64
    # the multiplier learns on the CPU: it moves at every update, by about cql_alpha_lr
    la = [float(g[f"u{u}_cql_log_alpha"][0]) for u in range(d["n_updates"])]
    assert la[0] != 0.0 and len(set(la)) == len(la)
    coef = lambda n: min(1.0, cfg.max_grad_norm / (n + 1e-6))  # noqa: E731
    assert any(coef(n) < 1.0 for u in range(d["n_updates"]) for n in g[f"u{u}_grad_norms"])
    g, d, cfg = CC.load_cql("plain")
    sa, sc = d["hidden"]
    assert d["activation"] == "tanh" and len(sa) == len(sc) == 3 and len(set(sa)) == 3 and len(set(sc)) == 3 and sa != sc
    assert not cfg.auto_alpha and not cfg.with_lagrange and not cfg.calibrated and d["R"] == 3
    assert (cfg.temperature, cfg.cql_weight, d["min_action"]) == (0.7, 5.0, 1.0)
    ra = g["u0_random_act"]
    assert ra.min() < -0.5 and ra.max() > 0.5 and np.abs(ra).max() <= 1.0                   # U(-1, 1)
    assert np.all(np.isnan(g["u0_stats"][[4, 5, 6]]))
    coef = lambda n: min(1.0, cfg.max_grad_norm / (n + 1e-6))  # noqa: E731
    assert any(coef(n) == 1.0 for u in range(d["n_updates"]) for n in g[f"u{u}_grad_norms"])
    for tag in CC.TAGS:
        assert os.path.getsize(os.path.join(CC.GOLDEN, f"cql_{tag}.npz")) <= 1 << 20


def test_logsumexp_runs_over_the_three_kinds_of_one_row():
    """cql_terms on values chosen by hand: three equal values give logsumexp = v / T + log 3 per row, and a calibration return
    above all of them gives ret / T + log 3 with no gradient to the Q arrays."""
    cfg = OC.CQLConfig(num_repeat_actions=2, temperature=0.5, cql_weight=1.0, with_lagrange=False)
    B, R, A = 3, 2, 4
    off = float(np.log(0.5 ** A))
    q = torch.full((B * R,), 2.0, dtype=torch.float64, requires_grad=True)
    qr = (torch.full((B * R,), 2.0, dtype=torch.float64) + off).requires_grad_(True)
    z = torch.zeros(B * R, dtype=torch.float64)
    qd, tgt = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    t = OC.cql_terms(qd, tgt, qr, q, q, z, z, None, None, A, cfg)
    assert abs(float(t["lse"].detach()) - (2.0 / 0.5 + np.log(3.0))) < 1e-12
    t = OC.cql_terms(qd, tgt, qr, q, q, z, z, torch.full((B,), 5.0, dtype=torch.float64), None, A, cfg)
    assert abs(float(t["lse"].detach()) - (5.0 / 0.5 + np.log(3.0))) < 1e-12
    assert float(torch.autograd.grad(t["cql"], q, allow_unused=True)[0].abs().max()) == 0.0


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, TS_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="random")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_cql.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for tag in CC.TAGS:
        f = f"cql_{tag}.npz"
        new, old = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(CC.GOLDEN, f))
        assert sorted(new.files) == sorted(old.files), f
        same = lambda a, b: np.array_equal(a, b, equal_nan=a.dtype.kind == "f")      # noqa: E731 (string arrays: no isnan)
        bad = [k for k in old.files if not same(new[k], old[k])]
        assert not bad, (f, bad[:5])
