"""CPU: tests/oracle_cbcq.py (the torch restatement the GPU parity tests compare against) replays the fixtures recorded from the
UNMODIFIED reference BCQ.update() on the CPU (tools/gen_golden_cbcq.py) at tests/test_oracle_cql.py's bars; where the reference
is mounted, the generator reproduces both files bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_shim
from tests import cbcq_common as BC
from tests import oracle_cbcq as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", BC.TAGS)
def test_cbcq_restatement_matches_reference(tag):
    """Statistics rtol 1e-5 / atol 1e-7, networks and lagged networks rtol 1e-5 / atol 1e-6, first moments rtol 1e-5 / atol 1e-8,
    second moments rtol 1e-5 / atol 1e-12 (test_cql_restatement_matches_reference's bars); the target and the critics' gradient
    norms before clipping at the statistics' bar."""
    g, d, cfg = BC.load_cbcq(tag)
    st = OB.CBCQState.create(*BC.init_of(d), cfg)
    for u in range(d["n_updates"]):
        col = {}
        out = OB.update_with_batch(st, cfg, **BC.batch_of(g, u), collect=col)
        np.testing.assert_allclose(BC.stats_vector(out), g[f"u{u}_stats"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(out["target"].numpy(), g[f"u{u}_target"], rtol=1e-5, atol=1e-7)
        if len(g[f"u{u}_grad_norms"]):
            norms = [OB.clip_coef(col[f"critic{k}_grads"], 1.0)[0] for k in (1, 2)]
            np.testing.assert_allclose(norms, g[f"u{u}_grad_norms"], rtol=1e-5)
        for name in BC.NETS + BC.LAGGED:
            np.testing.assert_allclose(OB.flatten(getattr(st, name)).numpy()[::61], g[f"u{u}_{name}"], rtol=1e-5, atol=1e-6, err_msg=name)
    for name in BC.NETS:
        opt = getattr(st, BC.OPTS[name])
        assert opt.step == int(g[f"adam_step_{name}"]) == d["n_updates"], name
        order = list(getattr(st, name).keys())
        np.testing.assert_allclose(OB.flatten({k: opt.m[k] for k in order}).numpy()[::61], g[f"adam_m_{name}"], rtol=1e-5, atol=1e-8, err_msg=name)
        np.testing.assert_allclose(OB.flatten({k: opt.v[k] for k in order}).numpy()[::61], g[f"adam_v_{name}"], rtol=1e-5, atol=1e-12, err_msg=name)


def test_fixtures_are_the_two_the_issue_describes():
    g, d, cfg = BC.load_cbcq("d4rl")
    assert (d["obs_dim"], d["act_dim"], d["latent_dim"], d["batch"], d["R"]) == (11, 3, 6, 64, 10) and d["n_updates"] == 3
    assert d["hidden"] == (256, 256) and d["vae_hidden"] == (512, 512) and cfg.activation == "relu"
    assert (cfg.phi, cfg.lmbda, cfg.max_action) == (0.05, 0.75, 1.0)
    assert cfg.pert_first_row                      # the example's plain MLP under Perturbation's `[0]`
    assert all(len(g[f"u{u}_grad_norms"]) == 0 for u in range(3))
    g, d, cfg = BC.load_cbcq("odd")
    assert (d["latent_dim"], d["batch"], d["R"]) == (5, 37, 3) and d["hidden"] == (64, 64, 64) and d["vae_hidden"] == (96, 96)
    assert (cfg.phi, cfg.lmbda, cfg.max_action) == (0.3, 1.0, 2.0) and cfg.critic1_lr != cfg.critic2_lr
    assert not cfg.pert_first_row and cfg.activation == "tanh" and cfg.critic1_max_grad_norm > 0
    assert any(g["done"][g[f"u{u}_indices"]].any() for u in range(3))
    coef = [min(1.0, cfg.critic1_max_grad_norm / (n + 1e-6)) for u in range(3) for n in g[f"u{u}_grad_norms"]]
    assert len(coef) == 6 and any(c < 1.0 for c in coef)            # the clip bites
    for tag in BC.TAGS:
        assert os.path.getsize(os.path.join(BC.GOLDEN, f"cbcq_{tag}.npz")) <= 1 << 20


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, TS_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="random")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_cbcq.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for tag in BC.TAGS:
        f = f"cbcq_{tag}.npz"
        new, old = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(BC.GOLDEN, f))
        assert sorted(new.files) == sorted(old.files), f
        same = lambda a, b: np.array_equal(a, b, equal_nan=a.dtype.kind == "f")      # noqa: E731 (string arrays: no isnan)
        bad = [k for k in old.files if not same(new[k], old[k])]
        assert not bad, (f, bad[:5])
