"""CPU: tests/oracle_bc.py (the torch restatement the GPU parity tests compare against) replays the fixtures recorded from the
UNMODIFIED reference OfflineImitationLearning.update() / OffPolicyImitationLearning.update() (tools/gen_golden_bc.py) at the
bars of tests/test_oracle_dcql.py (losses: 1e-6 relative); where the reference is mounted, the generator reproduces the files
bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle_dqn as OD
from oracle import ref_shim
from tests import bc_common as CC
from tests import oracle_bc as OB
from tianshou_amd import bc as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(CC.CASES))
def test_bc_restatement_matches_reference(case):
    s = CC.load(case)
    g, tag = s.g, s.tag
    cfg = OD.DQNConfig(lr=s.lr)
    st = OD.DQNState.create(s.params0, cfg)
    for u in range(s.n_updates):
        idx = g[f"{tag}u{u}_indices"]
        assert idx.shape == (s.batch,)
        loss = OB.update_with_batch(st, cfg, s.route, s.obs[idx], s.act[idx], s.max_action)
        np.testing.assert_allclose(loss, float(g[f"{tag}u{u}_loss"]), rtol=1e-6)
        np.testing.assert_allclose(CC.flat(st.params, s.order)[::CC.STRIDE], g[f"{tag}u{u}_params_strided"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(CC.biases(st.params, s.order), g[f"{tag}u{u}_biases"], rtol=1e-6, atol=1e-7)
    assert int(g[f"{tag}adam_step"]) == st.adam_step == s.n_updates
    np.testing.assert_allclose(CC.flat(st.adam_m, s.order)[::CC.STRIDE], g[f"{tag}adam_m_strided"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(CC.flat(st.adam_v, s.order)[::CC.STRIDE], g[f"{tag}adam_v_strided"], rtol=1e-5, atol=1e-12)


def test_fixtures_are_the_ones_the_generator_describes():
    a, c, da, db = (CC.load(k) for k in ("atari", "cartpole", "d4rl_a", "d4rl_b"))
    assert (a.c, a.h, a.w, a.n_act, a.batch) == (2, 44, 36, 3, 8) and a.obs.dtype == np.uint8
    assert (c.obs_dim, c.hidden, c.n_out) == (4, (64, 64), 2)
    assert (da.obs_dim, da.n_out, da.hidden, da.max_action, db.max_action) == (17, 6, (256, 256), 1.0, 2.5)
    assert a.n_act <= BC.MAX_ACT and c.n_out <= BC.MAX_ACT and da.n_out <= BC.MAX_ACT_DIM        # inside the engines' envelope
    assert float(np.abs(db.act).max()) > 1.0                  # the 2.5 fixture leaves [-1, 1]
    for f in CC.FILES:
        assert os.path.getsize(os.path.join(CC.GOLDEN, f)) <= 250_000, f


@pytest.mark.parametrize("route", OB.ROUTES)
def test_loss_of_the_restatement_against_float64_closed_form(route):
    """loss and d loss / d head bias of oracle_bc.gradients equal the closed forms of the two losses in float64: mean nll and
    sum_b (softmax - onehot) / B; mean squared error and sum_b 2 (a - a*) max_action (1 - tanh^2) / (B A)."""
    rng = np.random.default_rng(3)
    B = 7
    if route == "dqnet":
        p = OD.init_params(2, 44, 36, 3, 5)
        obs, act, bias = rng.integers(0, 256, size=(B, 2, 44, 36), dtype=np.uint8), rng.integers(0, 3, size=B), "fc2.b"
    else:
        n_out = 5 if route == "discrete" else 3
        p = OB.init_mlp_params(6, n_out, (32, 32), 5)
        obs, bias = rng.normal(size=(B, 6)).astype(np.float32), "ba"
        act = rng.integers(0, n_out, size=B) if route == "discrete" else rng.uniform(-2, 2, size=(B, n_out)).astype(np.float32)
    ma = 2.5
    loss, grads = OB.gradients(route, p, obs, act, ma)
    if route == "continuous":
        a = OB.forward(route, p, obs, ma).detach().double()
        t = a / ma
        tgt = torch.as_tensor(act).double()
        want = float(((a - tgt) ** 2).mean())
        g64 = (2.0 * (a - tgt) * ma * (1.0 - t * t)).sum(0) / a.numel()
    else:
        z = OB.forward(route, p, obs).detach().double()
        at = torch.as_tensor(act)
        want = float((torch.logsumexp(z, 1) - z[torch.arange(B), at]).mean())
        g64 = (torch.softmax(z, 1) - torch.nn.functional.one_hot(at, z.shape[1])).sum(0) / B
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert float((grads[bias].double() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, TS_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="random")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_bc.py")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for f in CC.FILES:
        new, old = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(CC.GOLDEN, f))
        assert sorted(new.files) == sorted(old.files), f
        same = lambda a, b: np.array_equal(a, b, equal_nan=a.dtype.kind == "f")      # noqa: E731 (string arrays: no isnan)
        bad = [k for k in old.files if not same(new[k], old[k])]
        assert not bad, (f, bad[:5])
