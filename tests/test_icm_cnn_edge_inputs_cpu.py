"""CPU: what needs no GPU of the CNN ICM edge inputs -- the refusals ts_icm_cnn_layout makes on the host (the other entry points
make the same ones through the same function, before any launch), the oracle identities the GPU edge tests rely on (dead
features, obs_next == obs, a single action), and the measured float32-vs-float64 distances the GPU bars quote."""
import ctypes

import numpy as np
import pytest
import torch

from tests import icm_cnn_cases as CS
from tests import oracle_icm_cnn as OC


def test_layout_refusals():
    from tianshou_amd import _lib
    from tianshou_amd import icm as IC

    lib, out = _lib.load(), (ctypes.c_int64 * 12)()

    def layout(c, h, w, a, mh, edit=None, mn_null=False, out_=out):
        _, mn = IC.net_descs(1, 1, [], "relu", mh)
        if edit:
            edit(mn)
        return lib.ts_icm_cnn_layout(_lib.i64(c), _lib.i64(h), _lib.i64(w), None if mn_null else ctypes.byref(mn), _lib.i64(a), out_)

    assert layout(4, 36, 36, 64, [512]) == _lib.TS_OK and out[1] == 64
    assert layout(4, 36, 36, 65, []) == _lib.TS_ERR_UNSUPPORTED and b"at most 64 actions" in lib.ts_last_error()
    assert layout(4, 36, 36, 0, []) == _lib.TS_ERR_INVALID_ARG
    assert layout(0, 36, 36, 2, []) == _lib.TS_ERR_INVALID_ARG
    assert layout(4, 35, 36, 2, []) == _lib.TS_ERR_INVALID_ARG and b"too small" in lib.ts_last_error()       # OH3 < 1
    assert layout(4, 36, 35, 2, []) == _lib.TS_ERR_INVALID_ARG and b"too small" in lib.ts_last_error()       # OW3 < 1
    assert layout(4, 7, 84, 2, []) == _lib.TS_ERR_INVALID_ARG
    assert layout(1, 36, 37, 2, []) == _lib.TS_ERR_INVALID_ARG and b"multiple of 4" in lib.ts_last_error()   # a shape the conv layer refuses
    assert layout(1, 36, 40, 2, []) == _lib.TS_OK
    assert layout(4, 36, 36, 2, [2000]) == _lib.TS_ERR_INVALID_ARG
    assert layout(4, 36, 36, 2, [0]) == _lib.TS_ERR_INVALID_ARG
    assert layout(4, 36, 36, 2, [], mn_null=True) == _lib.TS_ERR_INVALID_ARG
    assert layout(4, 36, 36, 2, [], out_=None) == _lib.TS_ERR_INVALID_ARG
    assert layout(4, 36, 36, 2, [], edit=lambda mn: setattr(mn, "n_hidden", 8)) == _lib.TS_ERR_INVALID_ARG
    assert layout(4, 36, 36, 2, [], edit=lambda mn: setattr(mn, "activation", 0)) == _lib.TS_ERR_UNSUPPORTED           # tanh models
    assert layout(4, 36, 36, 2, [], edit=lambda mn: setattr(mn, "flags", _lib.NetDesc.LAYERNORM)) == _lib.TS_ERR_UNSUPPORTED
    # without a workspace nothing runs
    assert lib.ts_icm_cnn_forward(None, *([None] * 14)) == _lib.TS_ERR_WORKSPACE


def test_engine_needs_a_gpu():
    from tianshou_amd import icm_cnn as ICC
    from tianshou_amd.icm import ICMConfig

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ICC.ICMCnnEngine(4, 36, 36, 6, [64], torch.zeros(10), ICMConfig())


def test_dead_features_get_no_gradient_in_autograd():
    """The GPU test's expectation: with conv3's bias at -1e6 on the odd channels those features are exactly 0 on every row and
    autograd gives their conv3 columns exactly zero gradient, while the pre-ReLU upstream gradient there is NOT zero -- the mask is
    what cuts it."""
    cs = CS.case("44x44_b63_a18")
    model = OC.cast(cs["model"], torch.float64)
    dead = torch.arange(64) % 2 == 1
    model[0][5][dead] = -1e6
    _, gs, _, _ = OC.grads(model, cs["obs"], cs["act"], cs["obs_next"], CS.W_FWD, CS.LR_SCALE)
    assert bool((gs[0][4][dead] == 0).all()) and bool((gs[0][5][dead] == 0).all()) and bool((gs[0][4][~dead] != 0).any())
    phi2 = OC.features(model[0], cs["obs_next"]).detach().requires_grad_(True)
    phi1 = OC.features(model[0], cs["obs"]).detach()
    p2h = OC.mlp(model[1], torch.cat([phi1, torch.nn.functional.one_hot(cs["act"], 18).double()], 1))
    loss = (0.5 * ((p2h - phi2) ** 2).sum(1)).mean()
    (up,) = torch.autograd.grad(loss, phi2)
    assert bool((up.reshape(-1, 64, 2, 2)[:, dead] != 0).any())


def test_obs_next_equal_obs_and_single_action():
    cs = CS.case("36x36")
    model = OC.cast(cs["model"], torch.float64)
    stats, gs, mse, act_hat = OC.grads(model, cs["obs"], cs["act"], cs["obs"], 0.5, 1.0)
    p2h, p2, _ = OC.parts(model, cs["obs"], cs["act"], cs["obs"])
    assert torch.equal(p2, OC.features(model[0], cs["obs"])) and bool(torch.isfinite(stats).all())
    one = CS.case("44x36_b1_a1")
    s1, g1, _, a1 = OC.grads(OC.cast(one["model"], torch.float64), one["obs"], one["act"], one["obs_next"], CS.W_FWD, CS.LR_SCALE)
    assert a1.shape == (1, 1) and float(s1[2]) == 0.0 and all(bool((g == 0).all()) for g in g1[2])
    assert torch.equal(OC.reward(cs["rew"], mse, 0.0), cs["rew"])


def test_float32_oracle_distances_behind_the_gpu_bars():
    """`pytest -s` prints them.  Everything but the post-step parameters at 84 x 84 stays a factor of eight under the default bars
    (1e-5); the first Adam step is a sign function of the gradient, and at F = 3136 the float32 oracle moves some entry 0.195 lr
    away from the float64 one -- tests/test_gpu_icm_cnn_edges.py quotes that number."""
    for name in CS.SHAPES:
        d = CS.distances(name)
        print(name, {k: f"{v:.2e}" for k, v in d.items()})
        for k in ("mse", "act_hat", "grad"):
            assert d[k] <= 1e-5 / 8, (name, k, d[k])
        assert np.isnan(d["stats"]) or d["stats"] <= 1e-5 / 8, (name, d["stats"])
        if name != "84x84":
            assert d["params_over_lr"] <= 0.02 / 8, (name, d["params_over_lr"])
    assert CS.distances("84x84")["params_over_lr"] == pytest.approx(0.195, abs=0.0006)
