"""CPU: tests/oracle_bcq.py (the torch restatement the GPU parity tests compare against) replays the fixtures recorded from
the UNMODIFIED reference DiscreteBCQ.update() (tools/gen_golden_bcq.py) at the bars of tests/test_oracle_dcql.py; where the
reference is mounted, the generator reproduces both files bit for bit and the stand-ins expose the real classes' attributes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import bcq_common as BC
from tests import oracle_bcq as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", BC.TAGS)
def test_bcq_restatement_matches_reference(tag):
    """Bars as tests/test_oracle_dcql.py.  The fixture holds what torch's CPU kernels computed on the host that recorded it, and
    this test replays them with torch's CPU kernels of the host it runs on; that test's docstring records how its last check,
    the Adam moments at rtol 1e-5, misses on a host with other convolution / GEMM code paths in entries where the three gradients
    nearly cancel.  On the recording host every bar here is met; the bar is kept as it is."""
    g, d, cfg, bstate = BC.load_bcq(tag)
    A = d["n_act"]
    st = OB.make_state(OB.init_params(d["c"], d["h"], d["w"], A, d["seed"]), cfg)
    for u in range(d["n_updates"]):
        idx = g[f"u{u}_indices"]
        acts: list = []
        ret = OB.preprocess(st, cfg, bstate, g["frames"], idx, 1, g["frames_next"], acts=acts)
        assert ret.shape == (d["batch"],) and len(acts) == 1
        assert np.array_equal(acts[0], g[f"u{u}_target_act"])           # row for row: the fixture's gaps make it well-defined
        np.testing.assert_allclose(ret, g[f"u{u}_returns"], rtol=1e-6, atol=1e-6)
        losses = OB.update_with_batch(st, cfg, g["frames"][idx], g["act"][idx], ret)
        for name, x in zip(BC.LOSS_NAMES, losses):
            np.testing.assert_allclose(x, float(g[f"u{u}_{name}"]), rtol=1e-5, err_msg=name)
        flat = torch.cat([st.params[k].reshape(-1) for k in OB.PARAM_ORDER]).numpy()
        np.testing.assert_allclose(flat[::BC.STRIDE], g[f"u{u}_params_strided"], rtol=1e-6, atol=1e-7)
        biases = torch.cat([st.params[k].reshape(-1) for k in OB.PARAM_ORDER if k.endswith(".b")]).numpy()
        np.testing.assert_allclose(biases, g[f"u{u}_biases"], rtol=1e-6, atol=1e-7)
        old = torch.cat([st.params_old[k].reshape(-1) for k in OB.LAGGED_ORDER]).numpy()
        np.testing.assert_allclose(old[::BC.STRIDE], g[f"u{u}_old_params_strided"], rtol=1e-6, atol=1e-7)
    assert int(g["adam_step"]) == st.adam_step
    m = torch.cat([st.adam_m[k].reshape(-1) for k in OB.PARAM_ORDER]).numpy()
    v = torch.cat([st.adam_v[k].reshape(-1) for k in OB.PARAM_ORDER]).numpy()
    np.testing.assert_allclose(m[::BC.STRIDE], g["adam_m_strided"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(v[::BC.STRIDE], g["adam_v_strided"], rtol=1e-5, atol=1e-12)


def test_fixtures_are_the_two_the_generator_describes():
    g, d, cfg, _ = BC.load_bcq("masked")
    assert (d["n_act"], d["seed"], cfg.gamma, cfg.n_step, cfg.target_update_freq, cfg.unlikely_action_threshold,
            cfg.imitation_logits_penalty) == (3, 23, 0.95, 3, 2, 0.9, 0.01)
    changed_min, _, dist, gap = g["conditions"]
    assert changed_min >= 0.25 and dist >= 1e-3 and gap >= 1e-3          # the generator's three conditions, as recorded
    g, d, cfg, _ = BC.load_bcq("plain")
    assert (d["n_act"], d["seed"], cfg.gamma, cfg.n_step, cfg.target_update_freq, cfg.unlikely_action_threshold,
            cfg.imitation_logits_penalty) == (4, 29, 0.9, 1, 1, 0.0, 0.5)
    assert g["conditions"][3] >= 1e-3 and g["conditions"][2] == -1.0     # a threshold of 0: no finite distance to log tau
    for tag in BC.TAGS:
        g, d, cfg, _ = BC.load_bcq(tag)
        assert (d["E"], d["slots"], d["steps"], d["c"], d["h"], d["w"], d["batch"], d["n_updates"]) == (3, 24, 30, 2, 44, 36, 24, 3)
        assert cfg.lr == 3e-4 and os.path.getsize(os.path.join(BC.GOLDEN, f"bcq_{tag}.npz")) <= 250_000


def test_masked_argmax_of_the_restatement_at_the_threshold():
    """The float32 comparison of the reference: a ratio equal to float32(log 0.3) is not masked, one ulp below is; a threshold
    of 0 masks nothing; a masked action with a larger Q loses; ties go to the first index."""
    lt = np.float32(np.log(0.3))
    assert float(lt) < np.log(0.3)                               # a comparison in double would mask the equal case
    q = torch.tensor([[0.0, 1.0]] * 3)
    lg = torch.tensor([[0.0, float(lt)], [0.0, float(np.nextafter(lt, np.float32(-np.inf)))], [0.0, -200.0]])
    assert OB.masked_argmax(q[:2], lg[:2], float(np.log(0.3))).tolist() == [1, 0]
    assert OB.masked_argmax(q[2:], lg[2:], -np.inf).tolist() == [1]
    assert OB.masked_argmax(torch.tensor([[2.0, 2.0, 3e38]]), torch.tensor([[0.0, 0.0, -5.0]]), float(np.log(0.3))).tolist() == [0]


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, TS_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="random")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_bcq.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for tag in BC.TAGS:
        f = f"bcq_{tag}.npz"
        new, old = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(BC.GOLDEN, f))
        assert sorted(new.files) == sorted(old.files), f
        same = lambda a, b: np.array_equal(a, b, equal_nan=a.dtype.kind == "f")      # noqa: E731 (string arrays: no isnan)
        bad = [k for k in old.files if not same(new[k], old[k])]
        assert not bad, (f, bad[:5])


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_bcq_standin_has_the_reference_surface():
    """tests/standin_bcq.py against the real DiscreteBCQ / DiscreteBCQPolicy / DiscreteActor / DQNet: parameter names, shapes and
    seeded values of the policy and of its lagged copy, the attributes the hooks read, the statistics' fields, the policy's
    forward pass; the hook bodies are the same code over either namespace."""
    ref_shim.install()
    import dataclasses

    import gymnasium as gym
    from tianshou.algorithm.imitation.discrete_bcq import DiscreteBCQ, DiscreteBCQPolicy, DiscreteBCQTrainingStats
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import DQNet
    from tianshou.utils.net.discrete import DiscreteActor

    from tests import standin_bcq as SB

    c, h, w, A = 2, 44, 36, 3
    torch.manual_seed(5)
    fn = DQNet(c=c, h=h, w=w, action_shape=A, features_only=True)
    rm, ri = (DiscreteActor(preprocess_net=fn, action_shape=A, hidden_sizes=[512], softmax_output=False) for _ in range(2))
    real = DiscreteBCQ(policy=DiscreteBCQPolicy(model=rm, imitator=ri, action_space=gym.spaces.Discrete(A),
                                                unlikely_action_threshold=0.4, target_update_freq=2),
                       optim=AdamOptimizerFactory(lr=1e-4), gamma=0.97, n_step_return_horizon=2, target_update_freq=2,
                       imitation_logits_penalty=0.03)
    torch.manual_seed(5)
    sf = SB.DQNetFeaturesOnly(c, h, w)
    sm, si = (SB.DiscreteActor(preprocess_net=sf, action_shape=A, hidden_sizes=[512], softmax_output=False) for _ in range(2))
    fake = SB.DiscreteBCQ(policy=SB.DiscreteBCQPolicy(model=sm, imitator=si, unlikely_action_threshold=0.4, target_update_freq=2),
                          lr=1e-4, gamma=0.97, n_step_return_horizon=2, target_update_freq=2, imitation_logits_penalty=0.03)
    for a, b, keys in ((real.policy, fake.policy, OB.TIANSHOU_KEYS),
                       (real.model_old.module, fake.model_old.module, [k[len("model."):] for k in OB.TIANSHOU_KEYS[:10]])):
        pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
        assert list(pa.keys()) == list(pb.keys()) == keys
        assert all(torch.equal(pa[k], pb[k]) for k in pa)                  # same construction order: same seeded init
    assert list(real.policy.state_dict().keys()) == list(fake.policy.state_dict().keys())     # the trunk a second time
    assert real.policy.model.preprocess is real.policy.imitator.preprocess and sm.preprocess is si.preprocess
    for name in ("gamma", "n_step", "freq", "_iter", "_weight_reg"):
        assert getattr(real, name) == getattr(fake, name), name
    assert real.policy._log_tau == fake.policy._log_tau
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam
    assert len(real.optim._optim.param_groups[0]["params"]) == len(fake.optim._optim.param_groups[0]["params"]) == 14
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm
    obs = np.random.default_rng(0).integers(0, 256, size=(5, c, h, w)).astype(np.float32)
    qa, _ = real.policy.model(obs)
    qb, _ = fake.policy.model(obs)
    assert torch.equal(qa, qb)
    names = lambda cls: {f.name for f in dataclasses.fields(cls)}      # noqa: E731
    want = {"loss", "q_loss", "i_loss", "reg_loss"}
    assert want <= names(DiscreteBCQTrainingStats) and want <= names(SB.DiscreteBCQTrainingStats)
    from tianshou_amd.integration import make_hip_discrete_bcq

    A_, B_ = make_hip_discrete_bcq(), make_hip_discrete_bcq(ref=SB)
    assert A_.__name__ == B_.__name__ == "HipDiscreteBCQ" and issubclass(A_, DiscreteBCQ) and issubclass(B_, SB.DiscreteBCQ)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_layout", "_hip_write_back", "_hip_check_model"):
        fa, fb = getattr(A_, name), getattr(B_, name)
        fa, fb = getattr(fa, "__wrapped__", fa), getattr(fb, "__wrapped__", fb)
        assert fa.__code__.co_code == fb.__code__.co_code, name
