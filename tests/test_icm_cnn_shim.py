"""CPU: the CNN ICM layer without a GPU -- ts_icm_cnn_layout (host only) against the python converters, the four feature-order
permutations, what `icm_cnn.describe_module` and the HipICMCnn constructor refuse, the seam's default in HipPPOCnn, the checkpoint
format, and the stand-ins against the real classes where the reference is mounted."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

from oracle import ref_shim
from tests import oracle_icm_cnn as OC
from tests import standin_icm as SM

REAL = ref_shim.reference_available()
C, H, W, A = 4, 44, 36, 3
F = OC.feature_dim(H, W)


def _feature_net(c=C, h=H, w=W):
    if REAL:
        ref_shim.install()
        from tianshou.env.atari.atari_network import DQNet

        return DQNet(c=c, h=h, w=w, action_shape=A, features_only=True).net
    return SM.DQNetFeatures(c, h, w).net[0]


def _model(feature_net=None, hidden_sizes=(64,), feature_dim=F, action_dim=A):
    ICM = SM.IntrinsicCuriosityModule
    if REAL:
        ref_shim.install()
        from tianshou.utils.net.discrete import IntrinsicCuriosityModule as ICM
    return ICM(feature_net=_feature_net() if feature_net is None else feature_net, feature_dim=feature_dim, action_dim=action_dim,
               hidden_sizes=list(hidden_sizes))


def _wrapped(kind="cnn"):
    from tianshou_amd.integration import make_hip_ppo_cnn, make_hip_ppo_discrete

    if kind == "cnn":
        trunk = SM.DQNetFeatures(C, H, W)
        return make_hip_ppo_cnn("ppo", ref=SM)(policy=SM.Policy(SM.DiscreteActor(trunk, A, softmax_output=False)), critic=SM.DiscreteCritic(trunk),
                                               device="cpu", lr=3e-4)
    from torch.distributions import Categorical

    trunk = SM.Net(5, [32, 32], nn.ReLU)
    return make_hip_ppo_discrete(ref=SM)(policy=SM.Policy(SM.DiscreteActor(trunk, A, softmax_output=True), dist_fn=Categorical),
                                         critic=SM.DiscreteCritic(trunk), device="cpu", lr=3e-4)


def _make(model=None, wrapped=None, **kw):
    from tianshou_amd.integration import make_hip_icm_cnn

    return make_hip_icm_cnn(ref=SM)(wrapped_algorithm=_wrapped() if wrapped is None else wrapped, model=_model() if model is None else model,
                                    lr=2e-3, lr_scale=0.3, reward_scale=0.5, forward_loss_weight=0.9, **kw)


def test_library_and_package_export_the_entry_points():
    import tianshou_amd
    from tianshou_amd import _lib

    names = ["ts_icm_cnn_layout", "ts_icm_cnn_forward", "ts_icm_cnn_reward", "ts_icm_cnn_grad", "ts_icm_cnn_apply"]
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names) and set(names) <= set(_lib.declared_symbols())
    assert {"make_hip_icm_cnn", "ICMCnnEngine"} <= set(tianshou_amd.__all__)


@pytest.mark.parametrize("c,h,w,a,mh", [(4, 36, 36, 6, [64]), (4, 44, 36, 3, []), (1, 44, 44, 64, [48, 80]), (4, 84, 84, 6, [512]), (3, 40, 36, 1, [7])])
def test_layout_matches_the_python_converters(c, h, w, a, mh):
    """Sizes and offsets of the five blocks, F, round trip, zero padding."""
    from tianshou_amd import _lib
    from tianshou_amd import icm as IC
    from tianshou_amd import icm_cnn as ICC

    out = (ctypes.c_int64 * 12)()
    _, mn = IC.net_descs(1, 1, [], "relu", mh)
    _lib.check(_lib.load().ts_icm_cnn_layout(_lib.i64(c), _lib.i64(h), _lib.i64(w), ctypes.byref(mn), _lib.i64(a), out))
    f = ICC.feature_dim(h, w)
    assert f == OC.feature_dim(h, w) and f % 64 == 0
    conv = [(8 * 8 * c + 1) * 32, (4 * 4 * 32 + 1) * 64, (3 * 3 * 64 + 1) * 64]
    models = [sum((IC._pad32(k) + 1) * IC._pad32(n) for k, n in zip(d[:-1], d[1:])) for d in ICC.model_dims(f, a, mh)]
    sizes = conv + models
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert list(out) == [sum(sizes), f] + [int(x) for i in range(5) for x in (offs[i], sizes[i])]
    model = OC.init_model(c, h, w, a, mh, seed=1)
    tensors = OC.flat_tensors(model)
    flat = ICC.flat_from_torch(tensors, c, h, w, a, mh, "cpu")
    pad = ICC.padding_mask(c, h, w, a, mh)
    assert flat.numel() == out[0] and bool((flat[pad] == 0).all()) and int((~pad).sum()) == sum(t.numel() for t in tensors)
    assert not bool(pad[:offs[3]].any())
    back = ICC.flat_to_torch(flat, c, h, w, a, mh)
    assert len(back) == len(tensors) and all(torch.equal(t, r) for t, r in zip(tensors, back))


@pytest.mark.parametrize("mh", [[], [24], [48, 80]])
def test_the_four_permutations_keep_the_function(mh):
    """The flat vector, read the way the engine reads it -- features in (h, w, channel) order, [K_pad + 1, N_pad] blocks -- computes
    what torch computes on (channel, h, w) features: rows [0, F) of the forward model's first layer, columns and bias of its last,
    rows [0, F) and [F, 2F) of the inverse model's first layer.  With hidden_sizes () the forward model is ONE layer: both."""
    from tianshou_amd import icm as IC
    from tianshou_amd import icm_cnn as ICC

    c, h, w, a = 2, 44, 44, 5
    f = OC.feature_dim(h, w)
    model = OC.cast(OC.init_model(c, h, w, a, mh, seed=2), torch.float64)
    g = torch.Generator().manual_seed(3)
    obs, nxt = (torch.randint(0, 256, (6, h, w, c), generator=g, dtype=torch.uint8) for _ in range(2))
    act = torch.randint(0, a, (6,), generator=g)
    p2h_t, p2_t, logits_t = OC.parts(model, obs, act, nxt)
    flat = ICC.flat_from_torch([t.float() for t in OC.flat_tensors(model)], c, h, w, a, mh, "cpu").double()
    # the engine's features: NHWC flatten of conv3's output
    def phi_engine(x):
        z = x.double().permute(0, 3, 1, 2)
        for i, (_, _, s) in enumerate(OC.CONVS):
            z = torch.relu(torch.nn.functional.conv2d(z, model[0][2 * i].float().double(), model[0][2 * i + 1].float().double(), stride=s))
        return z.permute(0, 2, 3, 1).flatten(1)

    def run_chain(x, dims, o):
        for i, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
            kp, np_ = IC._pad32(k), IC._pad32(n)
            blk = flat[o:o + (kp + 1) * np_].reshape(kp + 1, np_)
            x = torch.cat([x, torch.zeros(x.shape[0], kp - x.shape[1], dtype=x.dtype)], 1) @ blk[:kp] + blk[kp]
            x = x[:, :n]
            if i + 2 < len(dims):
                x = torch.relu(x)
            o += (kp + 1) * np_
        return x, o

    o = sum([(8 * 8 * c + 1) * 32, (4 * 4 * 32 + 1) * 64, (3 * 3 * 64 + 1) * 64])
    d_fwd, d_inv = ICC.model_dims(f, a, mh)
    phi1, phi2 = phi_engine(obs), phi_engine(nxt)
    p2h_e, o = run_chain(torch.cat([phi1, torch.nn.functional.one_hot(act, a).double()], 1), d_fwd, o)
    logits_e, o = run_chain(torch.cat([phi1, phi2], 1), d_inv, o)
    assert o == flat.numel()
    perm = ICC._feat_perm(h, w)
    np.testing.assert_allclose(phi2.numpy(), p2_t.numpy()[:, perm], rtol=1e-6)
    np.testing.assert_allclose(p2h_e.numpy(), p2h_t.detach().numpy()[:, perm], rtol=1e-5, atol=1e-6 * float(p2h_t.abs().max()))
    np.testing.assert_allclose(logits_e.numpy(), logits_t.detach().numpy(), rtol=1e-5, atol=1e-6 * float(logits_t.abs().max()))
    # ... so the mse, a sum over features, does not see the order
    np.testing.assert_allclose((0.5 * ((p2h_e - phi2) ** 2).sum(1)).numpy(), (0.5 * ((p2h_t - p2_t) ** 2).sum(1)).detach().numpy(), rtol=1e-5)


def test_describe_module_accepts_the_atari_model_and_names_what_it_refuses():
    from tianshou_amd import icm_cnn as ICC

    d = ICC.describe_module(_model(), C, H, W)
    assert (d["c"], d["n_act"], d["feature_dim"], d["model_hidden"]) == (C, A, F, [64])
    assert [tuple(t.shape) for t in d["tensors"]] == [(32, C, 8, 8), (32,), (64, 32, 4, 4), (64,), (64, 64, 3, 3), (64,), (64, F + A), (64,),
                                                      (F, 64), (F,), (64, 2 * F), (64,), (A, 64), (A,)]
    assert ICC.describe_module(_model())["feature_dim"] == F                      # before a buffer is seen: the frame size is open
    nested = nn.Sequential(_feature_net())                                         # nested, as DQNet(output_dim_added_layer=...).net holds it
    assert ICC.describe_module(_model(nested), C, H, W)["feature_dim"] == F
    assert ICC.describe_module(_model(hidden_sizes=()), C, H, W)["model_hidden"] == []

    def convs(*layers):
        return nn.Sequential(*layers)

    base = lambda: [nn.Conv2d(C, 32, 8, 4), nn.ReLU(), nn.Conv2d(32, 64, 4, 2), nn.ReLU(), nn.Conv2d(64, 64, 3, 1), nn.ReLU(), nn.Flatten()]  # noqa: E731
    with pytest.raises(NotImplementedError, match="found Conv2d, ReLU, Conv2d, ReLU, Conv2d, ReLU, Flatten, Linear"):
        ICC.describe_module(_model(convs(*base(), nn.Linear(F, F))), C, H, W)
    with pytest.raises(NotImplementedError, match="found Linear"):
        ICC.describe_module(_model(SM.MLP(5, F, [])), C, H, W)
    with pytest.raises(NotImplementedError, match="found Conv2d, ReLU, Conv2d, ReLU, Conv2d, Flatten"):
        ICC.describe_module(_model(convs(*base()[:5], nn.Flatten())), C, H, W)
    other = base()
    other[2] = nn.Conv2d(32, 64, 3, 2)
    with pytest.raises(NotImplementedError, match=r"conv2 must be Conv2d\(32, 64, 4, 2\) \(found Conv2d\(32, 64, kernel_size=\(3, 3\)"):
        ICC.describe_module(_model(convs(*other)), C, H, W)
    other = base()
    other[0] = nn.Conv2d(C, 32, 8, 4, padding=1)
    with pytest.raises(NotImplementedError, match=r"conv1 must be .* padding=\(1, 1\)"):
        ICC.describe_module(_model(convs(*other)), C, H, W)
    other = base()
    other[4] = nn.Conv2d(64, 64, 3, 1, bias=False)
    with pytest.raises(NotImplementedError, match="conv3 without bias"):
        ICC.describe_module(_model(convs(*other)), C, H, W)
    with pytest.raises(NotImplementedError, match=rf"conv1 must be Conv2d\(3, 32, 8, 4\) \(found Conv2d\({C}, 32"):
        ICC.describe_module(_model(), 3, H, W)
    with pytest.raises(NotImplementedError, match=rf"feature_dim / action_dim \({F + 64}, {A}\) do not match the networks' outputs \({F} = 64 OH3 OW3 on {H} x {W}"):
        ICC.describe_module(_model(feature_dim=F + 64), C, H, W)
    with pytest.raises(NotImplementedError, match=rf"do not match the networks' outputs \(64 = 64 OH3 OW3 on 36 x 36"):
        ICC.describe_module(_model(), C, 36, 36)
    with pytest.raises(NotImplementedError, match="20 x 36 frame is too small"):
        ICC.describe_module(_model(), C, 20, 36)
    with pytest.raises(NotImplementedError, match="must be 64 OH3 OW3"):
        ICC.describe_module(_model(feature_dim=100))
    tanh = _model()
    tanh.forward_model = SM.MLP(F + A, F, [64], activation=nn.Tanh)
    with pytest.raises(NotImplementedError, match="forward_model: the activation must be one of .'relu'. .found tanh"):
        ICC.describe_module(tanh, C, H, W)
    uneven = _model()
    uneven.inverse_model = SM.MLP(2 * F, A, [32])
    with pytest.raises(NotImplementedError, match=r"must share their hidden sizes \(found \[64\] and \[32\]\)"):
        ICC.describe_module(uneven, C, H, W)
    with pytest.raises(NotImplementedError, match="at most 64 actions .found 65"):
        ICC.describe_module(_model(action_dim=65), C, H, W)
    with pytest.raises(NotImplementedError, match="hidden widths up to 1024 are supported .found 2048"):
        ICC.describe_module(_model(hidden_sizes=(2048,)), C, H, W)
    with pytest.raises(NotImplementedError, match="found Linear without `feature_net`"):
        ICC.describe_module(nn.Linear(3, 3), C, H, W)


def test_class_part_and_seam():
    algo = _make()
    assert type(algo).__name__ == "HipICMCnn" and (algo.lr_scale, algo.reward_scale, algo.forward_loss_weight) == (0.3, 0.5, 0.9)
    assert algo._hip_icm == dict(c=C, n_act=A, feature_dim=F, model_hidden=[64])
    with pytest.raises(RuntimeError, match="frame size is known with the first buffer"):
        algo._hip_parts()
    algo._hip_frame = (C, H, W)
    (part,) = algo._hip_parts()
    assert part.name == "params" and part.moments == ("state_m", "state_v") and part.step == "optim_step" and part.optim is algo.optim
    assert len(part.params) == 14 and part.flat().numel() == sum(p.numel() for p in part.params) + int(
        __import__("tianshou_amd.icm_cnn", fromlist=["x"]).padding_mask(C, H, W, A, [64]).sum())
    w = algo.wrapped_algorithm
    assert w._hip_rewards(None, None) is None                                  # the seam's default: the mirror's own column
    w.__dict__["_hip_rew_source"] = "x"
    assert w._hip_rewards(None, None) == "x"
    with pytest.raises(NotImplementedError, match="HipPPOCnn or a HipA2CCnn .found HipPPODiscrete"):
        _make(wrapped=_wrapped("discrete"))
    with pytest.raises(NotImplementedError, match="found Linear"):
        _make(model=_model(SM.MLP(5, F, [])))
    from tianshou_amd.integration import make_hip_ppo_cnn

    trunk = SM.DQNetFeatures(C, H, W)
    a2c = make_hip_ppo_cnn("a2c", ref=SM)(policy=SM.Policy(SM.DiscreteActor(trunk, A, softmax_output=False)), critic=SM.DiscreteCritic(trunk),
                                          device="cpu", lr=3e-4)
    assert type(_make(wrapped=a2c).wrapped_algorithm).__name__ == "HipA2CCnn"


def test_the_vector_wrapper_still_refuses_the_cnn_pairing():
    """make_hip_icm is unchanged: a conv feature net and a HipPPOCnn are refused by name there."""
    from tianshou_amd.integration import make_hip_icm

    with pytest.raises(NotImplementedError, match="HipPPODiscrete or a HipA2CDiscrete .found HipPPOCnn"):
        make_hip_icm(ref=SM)(wrapped_algorithm=_wrapped(), model=_model(), lr=1e-3, lr_scale=1.0, reward_scale=0.01, forward_loss_weight=0.2)


def test_state_dict_keeps_the_reference_format():
    torch.manual_seed(3)
    hip = _make()
    trunk = SM.DQNetFeatures(C, H, W)
    plain_ppo = SM.PPO(policy=SM.Policy(SM.DiscreteActor(trunk, A, softmax_output=False)), critic=SM.DiscreteCritic(trunk))
    plain = SM.ICMOnPolicyWrapper(wrapped_algorithm=plain_ppo, model=_model(), lr=2e-3, lr_scale=0.3, reward_scale=0.5, forward_loss_weight=0.9)
    sd, nested = hip.state_dict(), "wrapped_algorithm._optimizers"
    assert set(sd) == set(plain.state_dict()) and nested in sd
    assert {k for k in sd if k.startswith("model.")} == {f"model.{n}" for n, _ in hip.model.named_parameters()}
    with torch.no_grad():
        for p in plain.parameters():
            p.add_(1.0)
    back = plain.state_dict()
    hip.load_state_dict(back, strict=True)                                     # the nested optimizer entry goes where it belongs
    assert hip._hip_engine is None and hip.wrapped_algorithm._hip_engine is None
    assert all(torch.equal(hip.state_dict()[k], back[k]) for k in sd if not k.endswith("_optimizers"))


@pytest.mark.skipif(not REAL, reason="needs the mounted reference")
def test_standins_match_the_real_classes():
    ref_shim.install()
    from tianshou.env.atari.atari_network import DQNet
    from tianshou.utils.net.discrete import IntrinsicCuriosityModule

    real_net = DQNet(c=C, h=H, w=W, action_shape=A, features_only=True)
    mine = SM.DQNetFeatures(C, H, W).net[0]
    assert int(real_net.output_dim) == F
    leaves = lambda net: [type(m).__name__ for m in net.modules() if not list(m.children())]  # noqa: E731
    assert leaves(real_net.net) == leaves(mine)
    assert [tuple(p.shape) for p in real_net.net.parameters()] == [tuple(p.shape) for p in mine.parameters()]
    real = IntrinsicCuriosityModule(feature_net=real_net.net, feature_dim=F, action_dim=A, hidden_sizes=[24])
    stand = SM.IntrinsicCuriosityModule(feature_net=mine, feature_dim=F, action_dim=A, hidden_sizes=[24])
    assert [tuple(v.shape) for v in real.state_dict().values()] == [tuple(v.shape) for v in stand.state_dict().values()]
    # the oracle's feature net IS the reference's module on the same tensors
    model = OC.init_model(C, H, W, A, [24], seed=5)
    with torch.no_grad():
        for p, t in zip(real_net.net.parameters(), model[0]):
            p.copy_(t)
    x = torch.randint(0, 256, (3, H, W, C), dtype=torch.uint8)
    assert torch.equal(real_net.net(x.permute(0, 3, 1, 2).float()), OC.features(model[0], x))
