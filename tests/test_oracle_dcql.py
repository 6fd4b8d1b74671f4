"""CPU: tests/oracle_dcql.py (the torch restatement the GPU parity tests compare against) replays the fixtures recorded from
the UNMODIFIED reference DiscreteCQL.update() (tools/gen_golden_dcql.py) at the bars of tests/test_oracle_iqn.py; where the
reference is mounted, the generator reproduces both files bit for bit and the stand-ins expose the real classes' attributes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import oracle_distq as OQ
from oracle import oracle_dqn as OD
from oracle import ref_shim
from tests import dcql_common as CC
from tests import oracle_dcql as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", CC.TAGS)
def test_dcql_restatement_matches_reference(tag):
    """Bars as tests/test_oracle_iqn.py.  The fixture holds what torch's CPU kernels computed on the host that recorded it, and
    this test replays them with torch's CPU kernels of the host it runs on: on the recording host every bar is met; on a host
    with another CPU (seen on a GPU machine's host: other convolution / GEMM code paths, another order of summation) every
    check passes up to the parameters, lagged parameters and sum-tree of all three updates, and the last one, the first Adam
    moments of "lagged" at rtol 1e-5 / atol 1e-8, misses in 21 of 2,824 sampled elements -- entries where the three
    gradients nearly cancel: largest absolute difference 2.6e-7 on a vector whose largest entry is 9.6e-2 (3e-6 of that scale), largest
    relative difference 9.2e-4.  tests/test_oracle_golden.py's DDPG case misses in the same way on that host (1 of 1,142
    elements, 5.3e-5 relative).  The bar is kept as it is."""
    g, d, cfg, bstate = CC.load_dcql(tag)
    A, N = d["n_act"], d["n_atoms"]
    lagged, prio_buf = cfg.target_update_freq > 0, d["prioritized"]
    assert (A * N) % 32 != 0 or tag == "single"            # "lagged": 63 live head columns, one padding column
    st = OD.DQNState.create(OQ.init_params(d["c"], d["h"], d["w"], A, N, d["seed"]), cfg.dqn())
    if prio_buf:
        tree = g["tree0"].copy()
        bound = 1
        while bound < d["E"] * d["slots"]:
            bound *= 2
        np.random.seed(d["seed"] + 7)
        mx, mn = 1.0, 1.0
    else:
        assert not any(k.endswith("is_weight") or k.endswith("tree") for k in g.files)
    for u in range(d["n_updates"]):
        idx = g[f"u{u}_indices"]
        w = None
        if prio_buf:
            scalar = np.random.rand(d["batch"]) * tree[1]
            assert np.array_equal(O._get_prefix_sum_idx(scalar, bound, tree), idx)
            w = O.per_get_weight(tree, bound, idx, mn, 0.4, True)
            np.testing.assert_allclose(w, g[f"u{u}_is_weight"], rtol=1e-4)
        ret = OQ.preprocess(st, cfg, bstate, g["frames"], idx, A, 1, g["frames_next"])
        assert ret.shape == (d["batch"], N)
        np.testing.assert_allclose(ret, g[f"u{u}_returns"], rtol=1e-6, atol=1e-6)
        (loss, qr_loss, cql_loss), prio = OC.update_with_batch(st, cfg, g["frames"][idx], g["act"][idx], ret, A, weight=w)
        np.testing.assert_allclose(prio.numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(loss, float(g[f"u{u}_loss"]), rtol=1e-5)
        np.testing.assert_allclose(qr_loss, float(g[f"u{u}_qr_loss"]), rtol=1e-5)
        np.testing.assert_allclose(cql_loss, float(g[f"u{u}_cql_loss"]), rtol=1e-5)
        flat = torch.cat([st.params[k].reshape(-1) for k in OD.PARAM_ORDER]).numpy()
        np.testing.assert_allclose(flat[::61], g[f"u{u}_params_strided"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(st.params["conv1.w"].numpy(), g[f"u{u}_conv1_w"], rtol=1e-6, atol=1e-7)
        biases = torch.cat([st.params[k].reshape(-1) for k in OD.PARAM_ORDER if k.endswith(".b")]).numpy()
        np.testing.assert_allclose(biases, g[f"u{u}_biases"], rtol=1e-6, atol=1e-7)
        if lagged:
            old = torch.cat([st.params_old[k].reshape(-1) for k in OD.PARAM_ORDER]).numpy()
            np.testing.assert_allclose(old[::61], g[f"u{u}_old_params_strided"], rtol=1e-6, atol=1e-7)
        if prio_buf:
            mx, mn = O.per_update_weight(tree, bound, idx, prio.numpy(), 0.6, mx, mn)
            np.testing.assert_allclose(tree, g[f"u{u}_tree"], rtol=1e-4)
    assert int(g["adam_step"]) == st.adam_step
    m = torch.cat([st.adam_m[k].reshape(-1) for k in OD.PARAM_ORDER]).numpy()
    v = torch.cat([st.adam_v[k].reshape(-1) for k in OD.PARAM_ORDER]).numpy()
    np.testing.assert_allclose(m[::61], g["adam_m_strided"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(v[::61], g["adam_v_strided"], rtol=1e-5, atol=1e-12)


def test_fixtures_are_the_two_the_generator_describes():
    g, d, cfg, _ = CC.load_dcql("lagged")
    assert (d["n_act"], d["n_atoms"], cfg.n_step, cfg.target_update_freq, cfg.min_q_weight, d["prioritized"]) == (3, 21, 3, 2, 10.0, True)
    g, d, cfg, _ = CC.load_dcql("single")
    assert (d["n_act"], d["n_atoms"], cfg.n_step, cfg.target_update_freq, cfg.min_q_weight, d["prioritized"]) == (4, 8, 1, 0, 0.5, False)
    for tag in CC.TAGS:
        g, d, _, _ = CC.load_dcql(tag)
        assert (d["E"], d["slots"], d["steps"], d["c"], d["h"], d["w"], d["batch"], d["n_updates"]) == (3, 24, 30, 2, 44, 36, 24, 3)
        assert os.path.getsize(os.path.join(CC.GOLDEN, f"dcql_{tag}.npz")) <= 250_000


def test_cql_term_of_the_restatement_against_float64_closed_form():
    """The added term of oracle_dcql.loss_terms on a small net: cql_loss and its gradient w.r.t. the head bias equal the
    closed form of the issue (softmax_a(q) - 1{a = act}) * min_q_weight / (B N), evaluated in float64."""
    c, h, w, A, N, B = 2, 44, 36, 3, 5, 7
    p = OQ.init_params(c, h, w, A, N, 3)
    rng = np.random.default_rng(0)
    obs = rng.integers(0, 256, size=(B, c, h, w), dtype=np.uint8)
    act = rng.integers(0, A, size=B)
    ret = rng.normal(size=(B, N)).astype(np.float32)
    grads = {}
    for mqw in (0.0, 2.5):
        cfg = OC.DiscreteCQLConfig(n_atoms=N, min_q_weight=mqw)
        q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        loss, qr_loss, cql_loss, _, dist = OC.loss_terms(q, cfg, obs, act, ret, A)
        loss.backward()
        grads[mqw] = q["fc2.b"].grad.double().view(A, N)
    qv = dist.detach().double().mean(2)
    lse = torch.logsumexp(qv, 1)
    want = float((lse - qv[torch.arange(B), torch.as_tensor(act)]).mean())
    assert abs(float(cql_loss.detach()) - want) <= 1e-5 * abs(want)
    g64 = (torch.softmax(qv, 1) - torch.nn.functional.one_hot(torch.as_tensor(act), A)).sum(0) * 2.5 / (B * N)
    got = grads[2.5] - grads[0.0]
    assert float((got - g64[:, None]).abs().max()) <= 1e-5 * float(g64.abs().max())


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, TS_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="random")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_dcql.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for tag in CC.TAGS:
        f = f"dcql_{tag}.npz"
        new, old = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(CC.GOLDEN, f))
        assert sorted(new.files) == sorted(old.files), f
        same = lambda a, b: np.array_equal(a, b, equal_nan=a.dtype.kind == "f")      # noqa: E731 (string arrays: no isnan)
        bad = [k for k in old.files if not same(new[k], old[k])]
        assert not bad, (f, bad[:5])


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_dcql_standin_has_the_reference_surface():
    """tests/standin_dcql.py against the real DiscreteCQL / QRDQNPolicy / QRDQNet: state_dict keys and shapes of the network
    and its lagged copy, the attributes the hooks read, the statistics' fields; the hook bodies are the same code over
    either namespace."""
    ref_shim.install()
    import dataclasses

    import gymnasium as gym
    from tianshou.algorithm.imitation.discrete_cql import DiscreteCQL, DiscreteCQLTrainingStats
    from tianshou.algorithm.modelfree.qrdqn import QRDQNPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import QRDQNet

    from tests import standin_dcql as SC

    c, h, w, A, N = 2, 44, 36, 3, 21
    torch.manual_seed(5)
    rnet = QRDQNet(c=c, h=h, w=w, action_shape=[A], num_quantiles=N)
    real = DiscreteCQL(policy=QRDQNPolicy(model=rnet, action_space=gym.spaces.Discrete(A)), optim=AdamOptimizerFactory(lr=1e-4),
                       min_q_weight=3.0, gamma=0.97, num_quantiles=N, n_step_return_horizon=2, target_update_freq=2)
    torch.manual_seed(5)
    fake = SC.DiscreteCQL(policy=SC.DiscreteQLearningPolicy(SC.QRDQNet(c, h, w, A, N)), lr=1e-4, min_q_weight=3.0, gamma=0.97,
                          num_quantiles=N, n_step_return_horizon=2, target_update_freq=2)
    for a, b in ((real.policy.model, fake.policy.model), (real.model_old.module, fake.model_old.module)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys()) == OD.TIANSHOU_KEYS
        assert all(torch.equal(sa[k], sb[k]) for k in sa)                  # same construction order: same seeded init
    assert [tuple(q.shape) for q in real.model_old.parameters()] == [tuple(q.shape) for q in fake.model_old.parameters()]
    for name in ("gamma", "n_step", "target_update_freq", "_iter", "num_quantiles", "min_q_weight"):
        assert getattr(real, name) == getattr(fake, name), name
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm
    names = lambda cls: {f.name for f in dataclasses.fields(cls)}      # noqa: E731
    assert {"loss", "qr_loss", "cql_loss"} <= names(DiscreteCQLTrainingStats) and {"loss", "qr_loss", "cql_loss"} <= names(SC.DiscreteCQLTrainingStats)
    SC.DiscreteCQLTrainingStats(loss=1.0, qr_loss=0.5, cql_loss=0.05)
    DiscreteCQLTrainingStats(loss=1.0, qr_loss=0.5, cql_loss=0.05)
    from tianshou_amd.integration import make_hip_discrete_cql

    A_, B_ = make_hip_discrete_cql(), make_hip_discrete_cql(ref=SC)
    assert A_.__name__ == B_.__name__ == "HipDiscreteCQL" and issubclass(A_, DiscreteCQL) and issubclass(B_, SC.DiscreteCQL)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_layout", "_n_atoms"):
        fa, fb = getattr(A_, name), getattr(B_, name)
        fa, fb = getattr(fa, "__wrapped__", fa), getattr(fb, "__wrapped__", fb)
        assert fa.__code__.co_code == fb.__code__.co_code, name
