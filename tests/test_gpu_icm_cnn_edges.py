"""GPU: the CNN ICM engine (tianshou_amd.icm_cnn over ts_icm_cnn_*) at the smallest shapes at which each piece can go wrong, against
tests/oracle_icm_cnn.py in float64 (tests/icm_cnn_cases.py builds the inputs and the reference once).

Bars: test_gpu_icm.py's -- mse / statistics / act_hat / rewards 1e-5 relative (act_hat with the absolute floor of 1e-5 of its
largest entry: a logit can sit near zero), the gradient 1e-5 of its largest entry, post-step parameters rtol 1e-5 / atol 0.02 lr.
The float32 oracle against the float64 oracle on the CPU on these very inputs (`python -m tests.icm_cnn_cases`) stays below
1.1e-6 on every one of the first four at every shape, so they hold everywhere, F = 3136 included.  The parameter bar does not at
84 x 84: after the FIRST Adam step every entry has moved by lr g / (|g| + eps), a sign function of the gradient, and the float32
oracle itself sits 0.195 lr from the float64 one there (an entry whose gradient is of the order of eps = 1e-8); the bar at that
shape is 8 x that, 1.56 lr, and the step is checked a second way that does not have this weakness: against torch.optim.Adam on
the ENGINE's gradient, where only the optimizer arithmetic differs."""
import numpy as np
import pytest
import torch

from tests import icm_cnn_cases as CS
from tests import oracle_icm_cnn as OC

pytestmark = pytest.mark.gpu

PARAM_ATOL_LR = {"84x84": 8 * 0.195}          # measured float32-vs-float64 oracle distance x 8 (module docstring); elsewhere 0.02


def engine(name, model=None, **cfg_kw):
    from tianshou_amd import icm_cnn as ICC
    from tianshou_amd.icm import ICMConfig

    cs = CS.case(name)
    c, h, w, a, mh = cs["dims"]
    kw = dict(lr_scale=CS.LR_SCALE, forward_loss_weight=CS.W_FWD, reward_scale=0.01, lr=CS.LR)
    kw.update(cfg_kw)
    flat = ICC.flat_from_torch(OC.flat_tensors(cs["model"] if model is None else model), c, h, w, a, mh, "cuda")
    return ICC.ICMCnnEngine(c, h, w, a, mh, flat, ICMConfig(**kw)), cs


def rows(cs, f32=False):
    obs, nxt = cs["obs"].cuda(), cs["obs_next"].cuda()
    if f32:
        obs, nxt = obs.float(), nxt.float()
    return obs, cs["act"].cuda(), nxt


def chains(eng, flat=None):
    t = eng.to_tensors(flat)
    n = 2 * (len(eng.model_hidden) + 1)
    return [t[:6], t[6:6 + n], t[6 + n:]]


@pytest.mark.parametrize("name", list(CS.SHAPES))
def test_shapes_against_the_oracle(name):
    """Forward, reward, gradient, statistics and one step at every frame size, B in {1, 63, 64, 65}, A in {1, 18, 33, 64}, hidden
    (), [48, 80], [512]; two identical calls are bit-identical; padding entries stay exactly zero through three updates."""
    from tianshou_amd import icm_cnn as ICC

    eng, cs = engine(name)
    ref = CS.reference(name)
    obs, act, nxt = rows(cs)
    rew = cs["rew"].cuda()
    mse, act_hat = eng.forward(obs, act, nxt)
    print(name, "mse rel", float(((mse.cpu().double() - ref["mse"]).abs() / ref["mse"]).max()))
    np.testing.assert_allclose(mse.cpu().numpy(), ref["mse"].numpy(), rtol=1e-5)
    np.testing.assert_allclose(act_hat.cpu().numpy(), ref["act_hat"].numpy(), rtol=1e-5, atol=1e-5 * float(ref["act_hat"].abs().max()))
    aug, mse_r = eng.reward(obs, act, nxt, rew, want_mse=True)
    assert torch.equal(mse, mse_r) and torch.equal(mse, eng.forward(obs, act, nxt, want_act_hat=False)[0])
    assert torch.equal(aug, rew + (mse * np.float32(0.01)).double())            # the float64 sum of a float32 product
    grad, grad2 = (torch.empty(eng.count, dtype=torch.float32, device="cuda") for _ in range(2))
    before = eng.params.clone()
    stats = eng.update(obs, act, nxt, grad_out=grad, apply=False)
    stats2 = eng.update(obs, act, nxt, grad_out=grad2, apply=False)
    assert torch.equal(stats, stats2) and torch.equal(grad, grad2) and torch.equal(eng.params, before) and eng.optim_step == 0
    c, h, w, a, mh = cs["dims"]
    pad = ICC.padding_mask(c, h, w, a, mh, "cuda")
    assert bool((grad[pad] == 0).all())
    np.testing.assert_allclose(stats.cpu().numpy(), ref["stats"].numpy(), rtol=1e-5, atol=1e-12)     # (A = 1: the inverse loss is 0)
    g_ref, g_eng = CS.cat(ref["grads"]), CS.cat(chains(eng, grad))
    print(name, "grad err / max", float(np.abs(g_eng - g_ref).max() / np.abs(g_ref).max()))
    np.testing.assert_allclose(g_eng, g_ref, rtol=0, atol=1e-5 * float(np.abs(g_ref).max()))
    assert torch.equal(eng.update(obs, act, nxt), stats) and eng.optim_step == 1
    p_eng = CS.cat(chains(eng))
    print(name, "param err / lr", float(np.abs(p_eng - CS.cat(ref["after"])).max() / CS.LR))
    np.testing.assert_allclose(p_eng, CS.cat(ref["after"]), rtol=1e-5, atol=PARAM_ATOL_LR.get(name, 0.02) * CS.LR)
    # the same step by torch.optim.Adam in float64 on the engine's own gradient: the optimizer arithmetic alone
    opt = OC.Optim(OC.cast(cs["model"], torch.float64), "adam", lr=CS.LR)
    opt.step([[t.double().cpu() for t in ch] for ch in chains(eng, grad)])
    np.testing.assert_allclose(p_eng, CS.cat(opt.model()), rtol=1e-5, atol=0.02 * CS.LR)
    for _ in range(2):
        eng.update(obs, act, nxt)
    assert eng.optim_step == 3
    assert bool((eng.params[pad] == 0).all()) and bool((eng.state_m[pad] == 0).all()) and bool((eng.state_v[pad] == 0).all())


def test_too_many_actions_and_bad_frames_are_refused():
    from tianshou_amd import _lib
    from tianshou_amd import icm_cnn as ICC
    from tianshou_amd.icm import ICMConfig

    with pytest.raises(_lib.EngineError) as e:
        ICC.ICMCnnEngine(4, 36, 36, 65, [], torch.zeros(8, device="cuda"), ICMConfig())
    assert e.value.code == _lib.TS_ERR_UNSUPPORTED and "at most 64 actions" in str(e.value)
    eng, cs = engine("36x36")
    obs, act, nxt = rows(cs)
    with pytest.raises(ValueError, match="NHWC"):
        eng.forward(obs[:, :35], act, nxt[:, :35])
    with pytest.raises(ValueError, match="differ in length"):
        eng.forward(obs, act[:3], nxt)


@pytest.mark.parametrize("n", [16, 17, 31])
def test_chunked_update_matches_one_pass(n):
    """N in {c, c + 1, 2c - 1} at chunk c = 16 against one pass: the same gradient and statistics up to the summation order (the
    default bars), bit-identical from run to run; the rows can come from a callable."""
    eng, cs = engine("36x36_b64_a33")
    obs, act, nxt = (x[:n] for x in rows(cs))
    g1, gc, gc2, gf = (torch.empty(eng.count, dtype=torch.float32, device="cuda") for _ in range(4))
    s1 = eng.update(obs, act, nxt, chunk=n, grad_out=g1, apply=False)
    sc = eng.update(obs, act, nxt, chunk=16, grad_out=gc, apply=False)
    sc2 = eng.update(obs, act, nxt, chunk=16, grad_out=gc2, apply=False)
    calls = []

    def gather(lo, hi):
        calls.append((lo, hi))
        return obs[lo:hi], act[lo:hi], nxt[lo:hi]

    sf = eng.update(gather, n=n, chunk=16, grad_out=gf, apply=False)
    assert calls == [(lo, min(lo + 16, n)) for lo in range(0, n, 16)]
    assert torch.equal(sc, sc2) and torch.equal(gc, gc2) and torch.equal(sc, sf) and torch.equal(gc, gf)
    if n == 16:
        assert torch.equal(s1, sc) and torch.equal(g1, gc)                      # one chunk either way
    np.testing.assert_allclose(sc.cpu().numpy(), s1.cpu().numpy(), rtol=1e-5)
    np.testing.assert_allclose(gc.cpu().numpy(), g1.cpu().numpy(), rtol=0, atol=1e-5 * float(g1.abs().max()))
    # ... and against the oracle on those n rows
    model = OC.cast(cs["model"], torch.float64)
    s_o, g_o, _, _ = OC.grads(model, obs.cpu(), act.cpu(), nxt.cpu(), CS.W_FWD, CS.LR_SCALE)
    np.testing.assert_allclose(sc.cpu().numpy(), s_o.numpy(), rtol=1e-5)
    np.testing.assert_allclose(CS.cat(chains(eng, gc)), CS.cat(g_o), rtol=0, atol=1e-5 * float(np.abs(CS.cat(g_o)).max()))
    # the step after a chunked pass moves the parameters once
    eng.update(obs, act, nxt, chunk=16)
    assert eng.optim_step == 1


@pytest.mark.parametrize("name", ["36x36", "44x36_b1_a1", "84x84"])
def test_uint8_and_float32_frames_are_bit_identical(name):
    eng, cs = engine(name)
    g8, g32 = (torch.empty(eng.count, dtype=torch.float32, device="cuda") for _ in range(2))
    m8, a8 = eng.forward(*rows(cs))
    m32, a32 = eng.forward(*rows(cs, f32=True))
    assert torch.equal(m8, m32) and torch.equal(a8, a32)
    s8 = eng.update(*rows(cs), grad_out=g8, apply=False)
    s32 = eng.update(*rows(cs, f32=True), grad_out=g32, apply=False)
    assert torch.equal(s8, s32) and torch.equal(g8, g32)


def test_degenerate_rows():
    """obs_next == obs rows; an action outside [0, A) is clamped into it; reward_scale 0 copies the rewards bit for bit."""
    eng, cs = engine("36x36")
    obs, act, nxt = rows(cs)
    nxt = nxt.clone()
    nxt[1], nxt[3] = obs[1], obs[3]
    model = OC.cast(cs["model"], torch.float64)
    grad = torch.empty(eng.count, dtype=torch.float32, device="cuda")
    stats = eng.update(obs, act, nxt, grad_out=grad, apply=False)
    s_o, g_o, m_o, _ = OC.grads(model, obs.cpu(), act.cpu(), nxt.cpu(), CS.W_FWD, CS.LR_SCALE)
    np.testing.assert_allclose(eng.forward(obs, act, nxt)[0].cpu().numpy(), m_o.numpy(), rtol=1e-5)
    np.testing.assert_allclose(stats.cpu().numpy(), s_o.numpy(), rtol=1e-5)
    np.testing.assert_allclose(CS.cat(chains(eng, grad)), CS.cat(g_o), rtol=0, atol=1e-5 * float(np.abs(CS.cat(g_o)).max()))
    a_bad, a_ok = act.clone(), act.clone()
    a_bad[0], a_bad[2], a_ok[0], a_ok[2] = -3, eng.n_act + 5, 0, eng.n_act - 1
    g_bad, g_ok = (torch.empty(eng.count, dtype=torch.float32, device="cuda") for _ in range(2))
    assert torch.equal(eng.update(obs, a_bad, nxt, grad_out=g_bad, apply=False), eng.update(obs, a_ok, nxt, grad_out=g_ok, apply=False))
    assert torch.equal(g_bad, g_ok) and torch.equal(eng.forward(obs, a_bad, nxt)[0], eng.forward(obs, a_ok, nxt)[0])
    rew = cs["rew"].cuda()
    eng.cfg.reward_scale = 0.0
    assert torch.equal(eng.reward(obs, act, nxt, rew), rew)


def test_dead_features_get_no_gradient():
    """conv3 with a strongly negative bias on half its channels: those features are exactly 0 on every row, so the gradient of
    those conv3 columns (weights and bias) is exactly 0 -- the direct mse term -d_p2h and the inverse model's input gradient both
    reach phi2 and must be cut by (phi > 0) -- and the rest matches autograd."""
    cs = CS.case("44x44_b63_a18")
    model = [[t.clone() for t in ch] for ch in cs["model"]]
    dead = torch.arange(64) % 2 == 1
    model[0][5][dead] = -1e6
    eng, _ = engine("44x44_b63_a18", model=model)
    obs, act, nxt = rows(cs)
    with torch.no_grad():
        phi = OC.features(OC.cast(model, torch.float64)[0], torch.cat([obs, nxt]).cpu()).reshape(-1, 64, 2, 2)
    assert bool((phi[:, dead] == 0).all()) and bool((phi[:, ~dead] > 0).any())
    grad = torch.empty(eng.count, dtype=torch.float32, device="cuda")
    stats = eng.update(obs, act, nxt, grad_out=grad, apply=False)
    g = chains(eng, grad)
    assert bool((g[0][4][dead] == 0).all()) and bool((g[0][5][dead] == 0).all())
    assert bool((g[0][4][~dead] != 0).any())
    s_o, g_o, _, _ = OC.grads(OC.cast(model, torch.float64), obs.cpu(), act.cpu(), nxt.cpu(), CS.W_FWD, CS.LR_SCALE)
    assert bool((g_o[0][4][dead] == 0).all())
    np.testing.assert_allclose(stats.cpu().numpy(), s_o.numpy(), rtol=1e-5)
    np.testing.assert_allclose(CS.cat(g), CS.cat(g_o), rtol=0, atol=1e-5 * float(np.abs(CS.cat(g_o)).max()))


def test_c_abi_refusals_come_before_any_launch():
    """A NULL pointer (nullable outputs excepted), B < 1, B > B_total, a batch whose stacked frames or conv1 output reach 2^31
    elements (the message says to split it), misaligned frames, a bad optimizer call: TS_ERR_INVALID_ARG with nothing launched --
    the oversized calls pass pointers to five rows and would fault otherwise."""
    import ctypes as C

    from tianshou_amd import _lib
    from tianshou_amd import icm as IC

    eng, cs = engine("84x84")
    obs, act, nxt = rows(cs)
    lib, ws, st = _lib.load(), eng._ws.handle, _lib.current_stream(eng.device)
    grad, sums = torch.zeros(eng.count, device="cuda"), torch.zeros(2, device="cuda")
    mse, stats = torch.zeros(5, device="cuda"), torch.zeros(3, device="cuda")
    P = _lib.ptr

    def grad_call(b, b_total, obs_p=None, grad_p=None, dims=None):
        return lib.ts_icm_cnn_grad(ws, P(eng.params), *(dims or eng._dims()), P(obs) if obs_p is None else obs_p, C.c_int(1), P(act), P(nxt),
                                   _lib.i64(b), _lib.i64(b_total), _lib.f64(0.2), _lib.f64(1.0), C.c_int(0), P(grad) if grad_p is None else grad_p,
                                   P(sums), st)

    bad = _lib.TS_ERR_INVALID_ARG
    assert grad_call(0, 5) == bad and grad_call(6, 5) == bad and b"B_total" in lib.ts_last_error()
    assert grad_call(5, 5, obs_p=C.c_void_p(0)) == bad and grad_call(5, 5, grad_p=C.c_void_p(0)) == bad
    assert grad_call(5, 5, obs_p=C.c_void_p(obs.data_ptr() + 1)) == bad and b"4-byte aligned" in lib.ts_last_error()
    too_many = 2 ** 31 // (2 * 84 * 84 * 4) + 1                                   # 2B h w c >= 2^31
    assert grad_call(too_many, too_many) == bad and b"split the batch" in lib.ts_last_error()
    _, mn = IC.net_descs(1, 1, [], "relu", [512])
    one_channel = (_lib.i64(1), _lib.i64(84), _lib.i64(84), C.byref(mn), _lib.i64(6))
    b1 = 2 ** 31 // (2 * 20 * 20 * 32) + 1                                        # 2B OH1 OW1 32 >= 2^31 while 2B h w c is not
    assert 2 * b1 * 84 * 84 < 2 ** 31 and grad_call(b1, b1, dims=one_channel) == bad and b"split the batch" in lib.ts_last_error()

    def forward_call(mse_p, act_hat_p):
        return lib.ts_icm_cnn_forward(ws, P(eng.params), *eng._dims(), P(obs), C.c_int(1), P(act), P(nxt), _lib.i64(5), mse_p, act_hat_p, st)

    assert forward_call(C.c_void_p(0), C.c_void_p(0)) == bad and forward_call(P(mse), C.c_void_p(0)) == _lib.TS_OK
    assert lib.ts_icm_cnn_reward(ws, P(eng.params), *eng._dims(), P(obs), C.c_int(1), P(act), P(nxt), _lib.i64(5), C.c_void_p(0), _lib.f64(0.1),
                                 C.c_void_p(0), C.c_void_p(0), st) == bad

    def apply_call(b_total=5, step=1, kind=0, grad_p=None):
        return lib.ts_icm_cnn_apply(ws, P(eng.params), P(eng.state_m), P(eng.state_v), _lib.i64(step), *eng._dims(), P(grad) if grad_p is None else grad_p,
                                    P(sums), _lib.i64(b_total), _lib.f64(0.2), _lib.f64(1.0), C.c_int32(kind), _lib.f64(-1.0), _lib.f64(0.9),
                                    _lib.f64(0.999), _lib.f64(1e-8), _lib.f64(0.0), _lib.f64(0.99), _lib.f64(0.0), C.c_int32(0), _lib.f64(0.0), P(stats), st)

    before = eng.params.clone()
    assert apply_call(b_total=0) == bad and apply_call(step=0) == bad and apply_call(kind=7) == bad and apply_call(grad_p=C.c_void_p(0)) == bad
    assert grad_call(5, 5) == _lib.TS_OK and apply_call() == _lib.TS_OK                # lr < 0: statistics only
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before) and torch.equal(stats, eng.update(obs, act, nxt, apply=False))
