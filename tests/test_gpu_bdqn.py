"""GPU: the BDQN engine (tianshou_amd.bdqn over ts_bdqn_*) against tests/oracle_bdqn.py in float64 and against the reference's
recorded runs (tests/golden/bdqn_*.npz), and the HipBDQN drop-in over the stand-ins (tests/standin_bdqn.py) on a plain and a
prioritized buffer.  Tolerances: tests/bdqn_common.py (the sibling MLP-chain tests'); the float32 oracle's own distance from
float64 is below half of each (tests/test_oracle_bdqn.py holds the figures)."""
import numpy as np
import pytest
import torch

from tests import bdqn_common as BC
from tests import oracle_bdqn as OB
from tests import standin_bdqn as SM

pytestmark = pytest.mark.gpu


def make_engine(g):
    from tianshou_amd import bdqn as BD

    dims, c = BC.dims_of(g), BC.cfg_of(g)
    p = BC.init_params(g)
    flat = BD.flat_from_torch([p[k] for k in BD.state_keys(dims)], *dims, "cuda")
    return BD.BDQNEngine(*dims, flat, BD.BDQNConfig(gamma=c["gamma"], target_update_freq=c["target_update_freq"], is_double=c["is_double"],
                                                    optimizer=c["optimizer"], lr=c["lr"]))


def cat(tensors) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors]).numpy()


@pytest.mark.parametrize("tag", BC.TAGS)
def test_engine_against_the_oracle_and_the_recorded_run(tag):
    from tianshou_amd import bdqn as BD

    g = BC.load(tag)
    dims, c = BC.dims_of(g), BC.cfg_of(g)
    keys, lr = OB.state_keys(dims), c["lr"]
    assert BD.state_keys(dims) == keys
    eng = make_engine(g)
    agent = OB.Agent(BC.init_params(g, torch.float64), dims, **c)
    pad = BD.padding_mask(dims, "cuda")
    for u in range(BC.n_updates(g)):
        b32, b64 = BC.batch_of(g, u, device="cuda"), BC.batch_of(g, u, torch.float64)
        # forward: q and the per-branch argmax of the online (and the lagged) network
        for old in ([False, True] if eng.params_old is not None else [False]):
            q, act = eng.forward(b32["obs_next"], old=old)
            q_o = agent.q(b64["obs_next"], old=old)
            np.testing.assert_allclose(q.cpu().numpy(), q_o.numpy(), rtol=BC.RTOL, atol=BC.Q_ATOL)
            assert torch.equal(act.cpu(), OB.argmax_lowest(q_o))
        ret = eng.target_q(b32["obs_next"], b32["rew"], b32["end"])
        ret_o = agent.target_q(b64["obs_next"], b64["rew"], b64["end"])
        np.testing.assert_allclose(ret.cpu().numpy(), ret_o.numpy(), rtol=BC.RTOL, atol=BC.Q_ATOL)
        np.testing.assert_allclose(ret.cpu().numpy(), g[f"u{u}_returns"], rtol=BC.RTOL, atol=BC.Q_ATOL)
        # gradient-only mode at unchanged parameters against float64 autograd
        before = (eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.adam_step, eng.iter)
        grad, loss_g, prio_g = eng.gradient(b32["obs"], b32["act"], ret, b32["weight"])
        assert torch.equal(eng.params, before[0]) and torch.equal(eng.adam_m, before[1]) and torch.equal(eng.adam_v, before[2])
        assert (eng.adam_step, eng.iter) == before[3:]
        g_o, loss_o, prio_o = agent.gradient(b64["obs"], b64["act"], ret_o, b64["weight"])
        ref = cat([g_o[k] for k in keys])
        np.testing.assert_allclose(cat(BD.flat_to_torch(grad, *dims)), ref, rtol=0, atol=BC.GRAD_RTOL * float(np.abs(ref).max()))
        assert not grad[pad].any()
        loss, prio = eng.update(b32["obs"], b32["act"], ret, b32["weight"])
        agent.update(b64["obs"], b64["act"], ret_o, b64["weight"])
        assert torch.equal(loss, loss_g) and torch.equal(prio, prio_g)
        np.testing.assert_allclose(float(loss), float(loss_o), rtol=BC.RTOL)
        np.testing.assert_allclose(float(loss), g[f"u{u}_loss"], rtol=BC.RTOL)
        np.testing.assert_allclose(prio.cpu().numpy(), prio_o.numpy(), rtol=BC.RTOL, atol=BC.prio_atol(g, u))
        np.testing.assert_allclose(prio.cpu().numpy(), g[f"u{u}_weight_out"], rtol=BC.RTOL, atol=BC.prio_atol(g, u))
        par = cat(eng.to_tensors())
        np.testing.assert_allclose(par, agent.cat().numpy(), rtol=BC.PAR_RTOL, atol=0.02 * lr)
        np.testing.assert_allclose(par[::BC.STRIDE], g[f"u{u}_params_strided"], rtol=BC.REC_RTOL, atol=0.02 * lr)
        if eng.params_old is not None:
            np.testing.assert_allclose(cat(eng.to_tensors(eng.params_old))[::BC.STRIDE], g[f"u{u}_old_strided"], rtol=BC.REC_RTOL, atol=0.02 * lr)
        assert not eng.params[pad].any() and not eng.adam_v[pad].any()
    v = cat(BD.flat_to_torch(eng.adam_v, *dims))[::BC.STRIDE]
    np.testing.assert_allclose(v, g["moment_v_strided"], rtol=BC.MOM_RTOL, atol=1e-6 * float(g["moment_v_strided"].max()))
    if "moment_m_strided" in g:
        m = cat(BD.flat_to_torch(eng.adam_m, *dims))[::BC.STRIDE]
        np.testing.assert_allclose(m, g["moment_m_strided"], rtol=BC.MOM_RTOL, atol=1e-6 * float(np.abs(g["moment_m_strided"]).max()))
    assert eng.iter == eng.adam_step == BC.n_updates(g)


# ---- HipBDQN over the stand-ins ---------------------------------------------------------------------------------------------
def build_buffer(g):
    d = g["dims"]
    E, slots, prioritized = int(d[6]), int(d[7]), bool(d[11])
    kw = dict(obs_shape=(int(d[0]),), act_shape=(int(d[3]),), act_dtype=np.int64)
    buf = SM.PrioritizedVectorReplayBuffer(E * slots, E, alpha=0.6, beta=0.4, **kw) if prioritized else SM.VectorReplayBuffer(E * slots, E, **kw)
    for k in ("obs", "obs_next", "act", "rew", "terminated", "truncated", "done"):
        getattr(buf, k)[:] = g[k]
    buf._lengths[:], buf.last_index[:] = g["buf_lengths"], g["buf_last_index"]
    for sb, n, ins in zip(buf.buffers, g["buf_lengths"], g["buf_insertion"]):
        sb._size, sb._insertion_idx = int(n), int(ins)
    assert np.array_equal(buf.unfinished_index(), g["unfinished"])
    if prioritized:
        tree = g["u0_tree_before"]
        buf.prio[:] = tree[tree.shape[0] // 2:][:buf.maxsize]
    return buf


def build_algo(g, **kw):
    from tianshou_amd.integration import make_hip_bdqn

    dims, c = BC.dims_of(g), BC.cfg_of(g)
    obs_dim, common, hv, ha, D, A, act = dims
    net = SM.BranchingNet(state_shape=obs_dim, num_branches=D, action_per_branch=A, common_hidden_sizes=list(common),
                          value_hidden_sizes=[hv] if hv else [], action_hidden_sizes=[ha] if ha else [],
                          activation=torch.nn.ReLU if act == "relu" else torch.nn.Tanh)
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.copy_(torch.as_tensor(g["init_" + k]))
    optim = (torch.optim.RMSprop, {}) if c["optimizer"] == "rmsprop" else None
    args = dict(policy=SM.BDQNPolicy(net), lr=c["lr"], optim=optim, gamma=float(g["cfg"][1]), target_update_freq=c["target_update_freq"],
                is_double=c["is_double"])
    args.update(kw)
    return make_hip_bdqn(ref=SM)(**args)


def run_update(algo, buf, g, u):
    buf.sample_indices = lambda n, idx=g[f"u{u}_indices"]: idx.copy()
    algo.policy.is_within_training_step = True
    try:
        return algo.update(buf, len(g[f"u{u}_indices"]))
    finally:
        algo.policy.is_within_training_step = False


def strided(module, keys):
    named = dict(module.named_parameters())
    return cat([named[k] for k in keys])[::BC.STRIDE]


@pytest.mark.parametrize("tag", BC.TAGS)
def test_hip_bdqn_against_the_recorded_run(tag):
    g = BC.load(tag)
    keys, lr = OB.state_keys(BC.dims_of(g)), BC.cfg_of(g)["lr"]
    algo, buf = build_algo(g), build_buffer(g)
    assert algo.gamma == float(g["cfg"][1]) != float(g["cfg"][2])            # the targets use _compute_return's default, as the reference's do
    seen = {}
    pre = type(algo)._preprocess_batch

    def spy(self, batch, buffer, indices):
        if hasattr(batch, "weight"):
            seen["is_weight"] = np.asarray(batch.weight).copy()
        out = pre(self, batch, buffer, indices)
        seen["returns"] = out.returns
        return out

    algo._preprocess_batch = spy.__get__(algo)
    for u in range(BC.n_updates(g)):
        stats = run_update(algo, buf, g, u)
        D, A = int(g["dims"][3]), int(g["dims"][4])
        assert seen["returns"].shape == (len(g[f"u{u}_indices"]), D, A) and seen["returns"].is_cuda
        assert seen["returns"].stride() == (1, 0, 0)                          # the [B] result expanded as a view
        np.testing.assert_allclose(seen["returns"][:, 0, 0].cpu().numpy(), g[f"u{u}_returns"], rtol=BC.RTOL, atol=BC.Q_ATOL)
        assert isinstance(stats.loss, float)
        np.testing.assert_allclose(stats.loss, g[f"u{u}_loss"], rtol=BC.RTOL)
        assert algo._iter == u + 1
        np.testing.assert_allclose(strided(algo.policy.model, keys), g[f"u{u}_params_strided"], rtol=BC.REC_RTOL, atol=0.02 * lr)
        if algo.model_old is not None:                                        # the lagged sync at the right update
            np.testing.assert_allclose(strided(algo.model_old.module, keys), g[f"u{u}_old_strided"], rtol=BC.REC_RTOL, atol=0.02 * lr)
        if tag == "per":                                                      # importance weights in, priorities out
            np.testing.assert_allclose(seen["is_weight"], g[f"u{u}_is_weight"], rtol=1e-6)
            idx, w = buf.weight_updates[-1]
            assert np.array_equal(idx, g[f"u{u}_indices"])
            np.testing.assert_allclose(w, np.abs(g[f"u{u}_weight_out"]) + BC.PER_EPS, rtol=BC.RTOL, atol=BC.prio_atol(g, u))
            tree = g[f"u{u}_tree_after"]
            np.testing.assert_allclose(buf.prio, tree[tree.shape[0] // 2:][:buf.maxsize], rtol=1e-4, atol=BC.prio_atol(g, u))
    # the optimizer state reaches torch.optim through state_dict()
    sd = algo.state_dict()
    opt = algo.optim._optim
    named = dict(algo.policy.model.named_parameters())
    second = "square_avg" if tag == "per" else "exp_avg_sq"
    v = cat([opt.state[named[k]][second] for k in keys])[::BC.STRIDE]
    np.testing.assert_allclose(v, g["moment_v_strided"], rtol=BC.MOM_RTOL, atol=1e-6 * float(g["moment_v_strided"].max()))
    if tag == "double":
        m = cat([opt.state[named[k]]["exp_avg"] for k in keys])[::BC.STRIDE]
        np.testing.assert_allclose(m, g["moment_m_strided"], rtol=BC.MOM_RTOL, atol=1e-6 * float(np.abs(g["moment_m_strided"]).max()))
    assert all(int(float(opt.state[named[k]]["step"])) == BC.n_updates(g) for k in keys)
    assert len(sd["_optimizers"]) == 1


@pytest.mark.parametrize("tag", BC.TAGS)
def test_hip_bdqn_resumes_from_a_torch_checkpoint(tag):
    """Two updates, state_dict(), a fresh algorithm loads it (parameters, lagged network, torch optimizer state) and makes the
    third update: bit-identical to the uninterrupted run -- the state round-trips through `_q_write_back` / `_q_load`."""
    import copy

    g = BC.load(tag)
    keys = OB.state_keys(BC.dims_of(g))
    a, buf_a = build_algo(g), build_buffer(g)
    for u in range(2):
        run_update(a, buf_a, g, u)
    sd = copy.deepcopy(a.state_dict())
    b, buf_b = build_algo(g), copy.deepcopy(buf_a)
    b.load_state_dict(sd)
    b._iter = a._iter                                                         # (a plain attribute: the reference does not checkpoint it either)
    assert b._hip_engine is None
    sa, sb = run_update(a, buf_a, g, 2), run_update(b, buf_b, g, 2)
    assert sa.loss == sb.loss
    assert np.array_equal(cat([dict(a.policy.model.named_parameters())[k] for k in keys]),
                          cat([dict(b.policy.model.named_parameters())[k] for k in keys]))
    if a.model_old is not None:
        assert np.array_equal(strided(a.model_old.module, keys), strided(b.model_old.module, keys))
    eng_a, eng_b = a._hip_engine_obj, b._hip_engine_obj
    assert torch.equal(eng_a.adam_m, eng_b.adam_m) and torch.equal(eng_a.adam_v, eng_b.adam_v) and eng_a.adam_step == eng_b.adam_step == 3


def test_hip_bdqn_foreign_write_rebuilds_the_engine():
    """A load into the policy is seen through the version counters: the engine is rebuilt from the torch state, the optimizer
    moments survive (they were flushed into torch.optim), and the learning rate is re-read at every update."""
    g = BC.load("double")
    algo, buf = build_algo(g), build_buffer(g)
    run_update(algo, buf, g, 0)
    eng = algo._hip_engine_obj
    assert eng is not None and eng.cfg.lr == BC.cfg_of(g)["lr"] and eng.cfg.gamma == float(g["cfg"][2])
    algo.policy.load_state_dict({k: v.clone() for k, v in algo.policy.state_dict().items()})
    assert algo._hip_engine is None
    algo.optim._optim.param_groups[0]["lr"] = 0.5 * BC.cfg_of(g)["lr"]
    run_update(algo, buf, g, 1)
    eng2 = algo._hip_engine_obj
    assert eng2 is not eng and eng2.adam_step == 2 and eng2.iter == 2 and eng2.cfg.lr == 0.5 * BC.cfg_of(g)["lr"]


def test_a_refused_update_leaves_the_lagged_network_and_the_counters_alone():
    g = BC.load("double")
    eng = make_engine(g)
    b = BC.batch_of(g, 0, device="cuda")
    eng.update(b["obs"], b["act"], b["rew"])                                  # iter 1: the next call (iter % 2 == 1) does not sync ...
    eng.update(b["obs"], b["act"], b["rew"])                                  # ... the one after it (iter 2) does
    old, state = eng.params_old.clone(), (eng.iter, eng.adam_step)
    assert not torch.equal(old, eng.params)
    with pytest.raises(ValueError, match="act must be"):
        eng.update(b["obs"], b["act"][:, :1], b["rew"])
    assert torch.equal(eng.params_old, old) and (eng.iter, eng.adam_step) == state == (2, 2)
