"""CPU: tests/oracle_iqn.py (the torch restatement the GPU parity tests compare against) replays the fixtures recorded
from the UNMODIFIED reference IQN.update() (tools/gen_golden_iqn.py) at the bars test_oracle_golden.py uses for qrdqn.npz;
where the reference is mounted, the real ImplicitQuantileNetwork's state dict equals the engine's layout table."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import oracle_dqn as OD
from oracle import ref_shim
from tests import iqn_common as IC
from tests import oracle_iqn as OI


@pytest.mark.parametrize("tag", IC.TAGS)
def test_iqn_restatement_matches_reference(tag):
    g, d, cfg, bstate = IC.load_iqn(tag)
    lagged = cfg.target_update_freq > 0
    st = OD.DQNState.create(OI.init_params(d["c"], d["h"], d["w"], d["n_act"], seed=d["seed"]), cfg.dqn())
    tree = g["tree0"].copy()
    bound = 1
    while bound < d["E"] * d["slots"]:
        bound *= 2
    np.random.seed(d["seed"] + 7)
    mx, mn = 1.0, 1.0
    for u in range(d["n_updates"]):
        idx = g[f"u{u}_indices"]
        scalar = np.random.rand(d["batch"]) * tree[1]
        assert np.array_equal(O._get_prefix_sum_idx(scalar, bound, tree), idx)
        w = O.per_get_weight(tree, bound, idx, mn, 0.4, True)
        np.testing.assert_allclose(w, g[f"u{u}_is_weight"], rtol=1e-4)
        tau_o, tau_t, tau_u = IC.taus_of(g, u, lagged)
        assert tau_o.shape == (d["batch"], d["n_online"]) and tau_u.shape == (d["batch"], d["n_online"])
        ret = OI.preprocess(st, cfg, bstate, g["frames"], idx, tau_o, tau_t, 1, g["frames_next"])
        assert ret.shape == (d["batch"], d["n_target"] if lagged else d["n_online"])
        np.testing.assert_allclose(ret, g[f"u{u}_returns"], rtol=1e-6, atol=1e-6)
        loss, prio = OI.update_with_batch(st, cfg, g["frames"][idx], g["act"][idx], ret, tau_u, weight=w)
        np.testing.assert_allclose(prio.numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(loss, float(g[f"u{u}_loss"]), rtol=1e-5)
        flat = torch.cat([st.params[k].reshape(-1) for k in OI.PARAM_ORDER]).numpy()
        np.testing.assert_allclose(flat[::61], g[f"u{u}_params_strided"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(st.params["conv1.w"].numpy(), g[f"u{u}_conv1_w"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(st.params["fc2.w"].numpy(), g[f"u{u}_fc2_w"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(st.params["emb.w"].numpy().reshape(-1)[::7], g[f"u{u}_emb_w_strided"], rtol=1e-6, atol=1e-7)
        biases = torch.cat([st.params[k].reshape(-1) for k in OI.PARAM_ORDER if k.endswith(".b")]).numpy()
        np.testing.assert_allclose(biases, g[f"u{u}_biases"], rtol=1e-6, atol=1e-7)
        if lagged:
            old = torch.cat([st.params_old[k].reshape(-1) for k in OI.PARAM_ORDER]).numpy()
            np.testing.assert_allclose(old[::61], g[f"u{u}_old_params_strided"], rtol=1e-6, atol=1e-7)
        mx, mn = O.per_update_weight(tree, bound, idx, prio.numpy(), 0.6, mx, mn)
        np.testing.assert_allclose(tree, g[f"u{u}_tree"], rtol=1e-4)
    assert int(g["adam_step"]) == st.adam_step
    m = torch.cat([st.adam_m[k].reshape(-1) for k in OI.PARAM_ORDER]).numpy()
    v = torch.cat([st.adam_v[k].reshape(-1) for k in OI.PARAM_ORDER]).numpy()
    np.testing.assert_allclose(m[::61], g["adam_m_strided"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(v[::61], g["adam_v_strided"], rtol=1e-5, atol=1e-12)


def test_engine_layout_table_and_key_order():
    """ts_iqn_layout (host only) against the oracle's shapes; TIANSHOU_KEYS of the product equals the oracle's list."""
    from tianshou_amd import iqn as I
    from tianshou_amd.build import build_library

    build_library()
    assert I.TIANSHOU_KEYS == OI.TIANSHOU_KEYS
    for c, h, w, A in ((4, 84, 84, 6), (2, 44, 36, 3), (1, 36, 36, 64)):
        lay = I.layout(c, h, w, A)
        sh = OI.param_shapes(c, h, w, A)
        ld = (A + 31) // 32 * 32
        sizes = [int(np.prod(sh[k + ".w"])) + int(np.prod(sh[k + ".b"])) for k in ("conv1", "conv2", "conv3", "emb", "fc1")]
        assert lay["F"] == OI.feature_dim(h, w) and lay["ld"] == ld
        assert list(np.diff(lay["off"])) == sizes + [513 * ld]
        assert I.param_count(c, h, w, A) == lay["total"]
    with pytest.raises(ValueError):
        I.param_count(4, 84, 84, 65)
    with pytest.raises(ValueError):
        I.param_count(4, 84, 84, 6, n_cos=32)


def test_flat_layout_round_trip_on_the_host():
    from tianshou_amd import iqn as I

    c, h, w, A = 2, 44, 36, 5
    p = OI.init_params(c, h, w, A, seed=2)
    flat = I.flat_from_torch([p[k] for k in OI.PARAM_ORDER], c, h, w, A, device="cpu")
    for k, t in zip(OI.PARAM_ORDER, I.flat_to_torch(flat, c, h, w, A)):
        assert torch.equal(t, p[k]), k
    # the embedding block in engine order: column f' = (h, w, c) of row k is We[k, f'], i.e. emb.w[(c, h, w), k]
    F = OI.feature_dim(h, w)
    off = (64 * c + 1) * 32 + 513 * 64 + 577 * 64
    emb = flat[off:off + 65 * F].reshape(65, F)
    oh, ow = OD.conv_out_hw(h, w)[-1]
    ch, y, x, k = 5, oh - 1, ow - 1, 17
    assert float(emb[k, (y * ow + x) * 64 + ch]) == float(p["emb.w"][(ch * oh + y) * ow + x, k])
    assert float(emb[64, (y * ow + x) * 64 + ch]) == float(p["emb.b"][(ch * oh + y) * ow + x])


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_reference_state_dict_matches_the_layout_table():
    ref_shim.install()
    from tianshou.env.atari.atari_network import DQNet
    from tianshou.utils.net.discrete import ImplicitQuantileNetwork

    c, h, w, A = 2, 44, 36, 3
    net = ImplicitQuantileNetwork(preprocess_net=DQNet(c=c, h=h, w=w, action_shape=[A], features_only=True), action_shape=[A],
                                  hidden_sizes=[512], num_cosines=64)
    sd = net.state_dict()
    assert list(sd.keys()) == OI.TIANSHOU_KEYS
    shapes = OI.param_shapes(c, h, w, A)
    for k_ref, k in zip(OI.TIANSHOU_KEYS, OI.PARAM_ORDER):
        assert tuple(sd[k_ref].shape) == shapes[k], k
    # the oracle's forward equals the real net's for the same fractions
    torch.manual_seed(0)
    obs = torch.randint(0, 256, (5, c, h, w)).float()
    torch.manual_seed(1)
    (logits, taus), _ = net(obs, sample_size=6)
    p = {k: sd[k_ref] for k_ref, k in zip(OI.TIANSHOU_KEYS, OI.PARAM_ORDER)}
    with torch.no_grad():
        ref = OI.logits(p, obs, taus)
    assert torch.allclose(logits, ref, rtol=1e-6, atol=1e-6)


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_iqn_standin_has_the_reference_surface():
    """tests/standin_iqn.py against the real IQN / IQNPolicy / ImplicitQuantileNetwork: state_dict keys and shapes of the
    network and its lagged copy, the attributes the hooks read; the hook bodies are the same code over either namespace."""
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.iqn import IQN, IQNPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.env.atari.atari_network import DQNet
    from tianshou.utils.net.discrete import ImplicitQuantileNetwork

    from tests import standin_iqn as SQ

    c, h, w, A = 4, 44, 36, 3
    torch.manual_seed(5)
    rnet = ImplicitQuantileNetwork(preprocess_net=DQNet(c=c, h=h, w=w, action_shape=[A], features_only=True), action_shape=[A],
                                   hidden_sizes=[512], num_cosines=64)
    real = IQN(policy=IQNPolicy(model=rnet, action_space=gym.spaces.Discrete(A), sample_size=9, online_sample_size=5,
                                target_sample_size=7), optim=AdamOptimizerFactory(lr=1e-4), gamma=0.97,
               n_step_return_horizon=2, target_update_freq=2)
    torch.manual_seed(5)
    fnet = SQ.ImplicitQuantileNetwork(preprocess_net=SQ.DQNetFeaturesOnly(c, h, w), action_shape=[A], hidden_sizes=[512])
    fake = SQ.IQN(policy=SQ.IQNPolicy(model=fnet, sample_size=9, online_sample_size=5, target_sample_size=7), lr=1e-4,
                  gamma=0.97, n_step_return_horizon=2, target_update_freq=2)
    for a, b in ((real.policy.model, fake.policy.model), (real.model_old.module, fake.model_old.module)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys()) == OI.TIANSHOU_KEYS
        assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
        assert all(torch.equal(sa[k], sb[k]) for k in sa)                  # same construction order: same seeded init
    for name in ("gamma", "n_step", "target_update_freq", "_iter"):
        assert getattr(real, name) == getattr(fake, name), name
    for name in ("sample_size", "online_sample_size", "target_sample_size"):
        assert getattr(real.policy, name) == getattr(fake.policy, name), name
    assert type(real.optim._optim) is type(fake.optim._optim) is torch.optim.Adam
    assert real.optim._max_grad_norm == fake.optim._max_grad_norm
    from tianshou_amd.integration import make_hip_iqn

    A_, B_ = make_hip_iqn(), make_hip_iqn(ref=SQ)
    for name in ("_preprocess_batch", "_update_with_batch", "_engine", "_layout", "_hip_check_model", "_hip_next_tau"):
        fa, fb = getattr(A_, name), getattr(B_, name)
        fa, fb = getattr(fa, "__wrapped__", fa), getattr(fb, "__wrapped__", fb)
        assert fa.__code__.co_code == fb.__code__.co_code, name
