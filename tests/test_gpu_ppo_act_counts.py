"""The 128-sample step kernels (ppo_step2_kernel / ppo_step1_kernel) at the real action count: the actor half is unrolled to
the next instantiated count (2, 4, 6, 8) instead of ACT_PAD = 8.  Every dropped term is an exact zero that the 8-wide loops
add last, so the exact-count arm must give the BITS of the padded one (`TS_PPO_NACT=8`: the kernel as it was before the count
became a template parameter) -- gradient of the last step, losses, parameters and both Adam moments under torch.equal -- and
both are held to the CPU oracle at the bars tests/test_gpu_ppo.py uses for these quantities (losses rtol 1e-5 / atol 2e-6;
gradient rtol 1e-4 / atol 5e-6 of its largest entry and 1e-5 of every block's own scale; parameters rtol 1e-4 / atol 2e-6;
moments rtol 1e-3 with atol 2e-7 of the largest first moment / 1e-10).

Rows: 300 (three workgroups, the last tile partly empty) and 128 (one full workgroup); three update() steps of the whole
batch each, once with the identity permutation and once with seeded ones.  `TS_PPO_STEPQ=0` puts these row counts on the
128-sample kernel (by default they run the feature-split one, which this parameter does not touch)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_ppo as OP

from tests.test_gpu_ppo import CFGS, assert_blocks_close, dev, random_problem, run_oracle

pytestmark = pytest.mark.gpu

N_ENV, REPEAT = 4, 3
CASES = [(17, a) for a in range(1, 9)] + [(3, 3), (3, 6)]       # act 5 and 7 round up to 6 and 8, 1 and 3 to 2 and 4


def make_perms(n, kind):
    if kind == "identity":
        return [np.arange(n) for _ in range(REPEAT)]
    rng = np.random.default_rng(7 * n + 1)
    return [rng.permutation(n) for _ in range(REPEAT)]


def engine_run(setenv, params, data, unf, obs_dim, act_dim, kw, perms, nact8):
    """Three whole-batch steps on the 128-sample kernel -> (gradient of the last step, losses, params, adam_m, adam_v)."""
    from tianshou_amd import ppo as P

    setenv("TS_PPO_STEPQ", "0")
    setenv("TS_PPO_NACT", "8" if nact8 else None)
    eng = P.PPOEngine(obs_dim, act_dim, OP.flatten_params(params).cuda(), P.PPOConfig(**kw))
    b = eng.preprocess(dev(data["obs"]), dev(data["obs_next"]), dev(data["act"]), dev(data["rew"]),
                       dev(data["terminated"]), dev(data["truncated"]), dev(unf))
    losses, steps, grads = eng.update(b, None, REPEAT, perms, want_grad=True)
    assert steps == REPEAT
    torch.cuda.synchronize()
    return grads.clone(), losses.clone(), eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()


def set_env(name, value):
    import os

    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


@pytest.fixture
def clean_env():
    import os

    saved = {k: os.environ.get(k) for k in ("TS_PPO_STEPQ", "TS_PPO_NACT")}
    yield set_env
    for k, v in saved.items():
        set_env(k, v)


@functools.lru_cache(maxsize=None)
def reference(obs_dim, act_dim, n, kind, cfg_name="mujoco", max_action=None):
    """The problem and the oracle's three steps on it (computed once per case).  The rewards get a mean of 1, so that the
    returns sit above the critic's values: c_bv is a block of ONE entry, the mean of the value-loss derivatives, and around
    zero-mean returns it cancels to ~1 / sqrt(n) of its terms -- at 300 rows the 1e-5 bar of a block's own scale would then
    measure the fp32 rounding of a sum of O(1) terms (~1e-7) against a number that is small by accident (7e-3 in one case:
    1.8e-5, on the critic's half, which the action count does not touch).  tests/test_gpu_ppo_wgrad_shapes.py shifts its
    returns for the same reason."""
    params, data = random_problem(n, obs_dim, act_dim, seed=100 * obs_dim + 10 * act_dim + n % 7)
    data = dict(data, rew=data["rew"] + 1.0)
    kw = dict(CFGS[cfg_name])
    if max_action is not None:
        kw["max_action"] = max_action
    perms = make_perms(n, kind)
    st, pre, losses_o, grads_o, unf = run_oracle(params, data, OP.PPOConfig(max_batchsize=4096, **kw), None, REPEAT, perms, N_ENV)
    flat = lambda d: torch.cat([d[k].reshape(-1) for k in OP.PARAM_ORDER]).numpy()      # noqa: E731
    return params, data, unf, kw, perms, dict(grads=grads_o.numpy(), losses=losses_o, params=OP.flatten_params(st.params).numpy(),
                                              adam_m=flat(st.adam_m), adam_v=flat(st.adam_v))


def assert_arms_equal(exact, padded):
    for name, a, c in zip(("gradient", "losses", "params", "adam_m", "adam_v"), exact, padded):
        assert torch.equal(a, c), f"{name}: the exact-count arm differs from the TS_PPO_NACT=8 arm in {int((a != c).sum())} entries"


def assert_matches_oracle(run, ref, obs_dim, act_dim):
    grads, losses, params, adam_m, adam_v = (t.cpu().numpy() for t in run)
    np.testing.assert_allclose(losses, ref["losses"], rtol=1e-5, atol=2e-6)
    gscale = float(np.abs(ref["grads"]).max())
    np.testing.assert_allclose(grads, ref["grads"], rtol=1e-4, atol=5e-6 * max(gscale, 1.0))
    assert_blocks_close(grads, ref["grads"], obs_dim, act_dim)
    np.testing.assert_allclose(params, ref["params"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(adam_m, ref["adam_m"], rtol=1e-3, atol=max(1e-7, 2e-7 * float(np.abs(ref["adam_m"]).max())))
    np.testing.assert_allclose(adam_v, ref["adam_v"], rtol=1e-3, atol=1e-10)


@pytest.mark.parametrize("kind", ["identity", "seeded"])
@pytest.mark.parametrize("n", [300, 128])
@pytest.mark.parametrize("obs_dim,act_dim", CASES)
def test_exact_count_arm_equals_padded_arm_and_oracle(clean_env, obs_dim, act_dim, n, kind):
    params, data, unf, kw, perms, ref = reference(obs_dim, act_dim, n, kind)
    exact = engine_run(clean_env, params, data, unf, obs_dim, act_dim, kw, perms, nact8=False)
    padded = engine_run(clean_env, params, data, unf, obs_dim, act_dim, kw, perms, nact8=True)
    assert_arms_equal(exact, padded)
    assert_matches_oracle(exact, ref, obs_dim, act_dim)


def test_bounded_actor_at_six_actions(clean_env):
    """max_action > 0 (the tanh bound on mu and its derivative inside the per-action loops), act 6.  The bounded kernels are
    instantiated at ACT_PAD only, so both arms run the same kernel here: this pins that the dispatch by action count leaves
    the bounded path where it was, and holds it to the oracle."""
    params, data, unf, kw, perms, ref = reference(17, 6, 300, "seeded", max_action=1.5)
    exact = engine_run(clean_env, params, data, unf, 17, 6, kw, perms, nact8=False)
    padded = engine_run(clean_env, params, data, unf, 17, 6, kw, perms, nact8=True)
    assert_arms_equal(exact, padded)
    assert_matches_oracle(exact, ref, 17, 6)


def test_a2c_at_two_actions(clean_env):
    params, data, unf, kw, perms, ref = reference(17, 2, 300, "seeded", cfg_name="a2c")
    exact = engine_run(clean_env, params, data, unf, 17, 2, kw, perms, nact8=False)
    padded = engine_run(clean_env, params, data, unf, 17, 2, kw, perms, nact8=True)
    assert_arms_equal(exact, padded)
    assert_matches_oracle(exact, ref, 17, 2)


@pytest.mark.parametrize("nets", [1, 2])
def test_one_network_kernel_at_three_actions(clean_env, nets):
    """ppo_step1_kernel (nets = 1: the actor's half alone, 2: the critic's): the two arms only -- the oracle has no such mode,
    and tests/test_gpu_ppo.py pins this kernel to the two-network one."""
    params, data, unf, kw, perms, _ = reference(17, 3, 300, "seeded")
    kw = dict(kw, nets=nets)
    exact = engine_run(clean_env, params, data, unf, 17, 3, kw, perms, nact8=False)
    padded = engine_run(clean_env, params, data, unf, 17, 3, kw, perms, nact8=True)
    assert_arms_equal(exact, padded)
    assert bool(exact[0].abs().sum() > 0)
