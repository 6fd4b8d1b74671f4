"""The tail of a PPO step -- ppo_reduce_slabs_kernel (column sums of the gradient slabs, entropy) and ppo_adam_kernel (clip,
optimizer step, loss report) -- at the edges of what the reduction starts in front of its barrier: the slab counts on both
sides of the all-loads-in-flight path (a multiple of 32 up to 512), the entropy terms held one per lane, the column ->
parameter map of both slab layouts; and the loss report switched off (ts_ppo_update with and without `losses_out`).

Every case drives the C ABI directly: three gradient steps, each a ts_ppo_grad (step + reduction, `parts` path) followed by a
one-step ts_ppo_update (`losses` path) on the same parameters.  What is asserted here:
  * parts[3] of ts_ppo_grad equals losses[3] of ts_ppo_update bit for bit, and both are the entropy
    sum_k (0.5 + 0.5 log(2 pi) + sigma_param[k]) evaluated in float64 to 1e-6 absolute (float32 rounding of at most eight
    terms of magnitude <= 3: a sanity bound; sigma_param differs per action, so a wrong lane or order shows);
  * ts_ppo_update without `losses_out` leaves the parameters and both moments as with it;
  * with TS_PARENT_LIB naming a libtsengine.so built from the parent commit (loaded beside this tree's, like TS_LIB_PATH):
    gradient, parts, losses, parameters, adam_m and adam_v of all three steps equal the parent's bit for bit.
The gradient's value itself is held to the oracle by tests/test_gpu_ppo.py, test_gpu_ppo_act_counts.py and
test_gpu_ppo_wgrad_shapes.py."""
import contextlib
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import oracle_ppo as OP

from tests.test_gpu_ppo import random_problem

pytestmark = pytest.mark.gpu

STEPS = 3
# (obs, act, rows, TS_PPO_STEPQ, permutations).  TS_PPO_STEPQ=0 puts the row count on the 128-sample kernel: one slab per
# 128 rows; unset, rows this few run the feature-split kernel, whose slabs have the other column layout.
SLAB_CASES = [
    (17, 6, 128, "0", "identity"),      # 1 slab
    (17, 6, 300, "0", "seeded"),        # 3 slabs, the last tile partly empty
    (17, 6, 2176, "0", "seeded"),       # 17 slabs: one thread of a column takes two, the others one
    (17, 6, 4096, "0", "identity"),     # 32 slabs: the first count with every load in flight
    (17, 6, 4224, "0", "seeded"),       # 33 slabs: the general loop again
]
SLABS = {128: 1, 300: 3, 2176: 17, 4096: 32, 4224: 33}
ACT_CASES = [(17, 1, 300, "0", "seeded"), (17, 8, 300, "0", "seeded"), (3, 3, 300, "0", "identity")]
STEPQ_CASE = (17, 6, 300, None, "seeded")
CASES = SLAB_CASES + ACT_CASES + [STEPQ_CASE]
case_id = lambda c: f"obs{c[0]}-act{c[1]}-rows{c[2]}-stepq{c[3]}-{c[4]}"      # noqa: E731


@contextlib.contextmanager
def stepq_env(value):
    saved = os.environ.get("TS_PPO_STEPQ")
    try:
        if value is None:
            os.environ.pop("TS_PPO_STEPQ", None)
        else:
            os.environ["TS_PPO_STEPQ"] = value
        yield
    finally:
        if saved is None:
            os.environ.pop("TS_PPO_STEPQ", None)
        else:
            os.environ["TS_PPO_STEPQ"] = saved


def sigma_offset(obs_dim, act_dim):
    from tianshou_amd import ppo as P

    off = 0
    for k in P.PARAM_ORDER:
        if k == "a_sigma":
            return off
        off += int(np.prod(P.param_shapes(obs_dim, act_dim)[k]))
    raise AssertionError("a_sigma not in the layout")


@functools.lru_cache(maxsize=None)
def problem(obs_dim, act_dim, rows, kind):
    """Seeded inputs of one case (host tensors, computed once): parameters with sigma_param = -1.5 .. 0.5 over the actions, a
    batch whose log pi_old / V_old lie around the policy's own (the ratios stay moderate), the steps' permutations."""
    from tianshou_amd import ppo as P

    seed = 1000 * obs_dim + 100 * act_dim + rows
    params, data = random_problem(rows, obs_dim, act_dim, seed=seed)
    flat = OP.flatten_params(params).clone()
    so = sigma_offset(obs_dim, act_dim)
    flat[so:so + act_dim] = torch.linspace(-1.5, 0.5, act_dim) if act_dim > 1 else torch.tensor([-1.5])
    obs, act = torch.from_numpy(data["obs"]), torch.from_numpy(data["act"])
    v, lp = P.infer(flat.cuda(), obs_dim, act_dim, obs.cuda(), act.cuda(), want_v=True, want_logp=True)
    g = torch.Generator().manual_seed(seed + 7)
    r = lambda: torch.randn(rows, generator=g)                 # noqa: E731
    batch = dict(obs=obs, act=act, adv=r(), returns=v.cpu() + 1.0 + r(), logp_old=lp.cpu() + 0.1 * r(), v_s=v.cpu() + 0.1 * r())
    rng = np.random.default_rng(seed + 11)
    perms = None if kind == "identity" else [torch.from_numpy(rng.permutation(rows)) for _ in range(STEPS)]
    return flat, batch, perms


class Arm:
    """One libtsengine.so with a workspace of its own."""

    def __init__(self, lib):
        self.lib = lib
        lib.ts_last_error.restype = C.c_char_p
        lib.ts_ppo_param_count.restype = C.c_int64
        lib.ts_ppo_record_width.restype = C.c_int64
        self.ws = C.c_void_p(0)
        self.check(lib.ts_workspace_create(C.byref(self.ws), C.c_int(0), C.c_size_t(0)))

    def check(self, rc):
        assert rc == 0, f"libtsengine error {rc}: {self.lib.ts_last_error().decode('utf-8', 'replace')}"

    def close(self):
        torch.cuda.synchronize()
        self.lib.ts_workspace_destroy(self.ws)

    def plan(self, obs_dim, act_dim, rows):
        """-> (variant, slabs) of ts_ppo_step_plan under the current environment."""
        v, s = C.c_int32(-1), C.c_int32(-1)
        self.check(self.lib.ts_ppo_step_plan(C.c_int64(obs_dim), C.c_int64(act_dim), C.c_int64(rows), C.c_int32(0), C.byref(v), None,
                                             C.byref(s)))
        return v.value, s.value

    def run(self, case, with_losses=True):
        from tianshou_amd import _lib
        from tianshou_amd import ppo as P

        obs_dim, act_dim, rows, stepq, kind = case
        flat, batch, perms = problem(obs_dim, act_dim, rows, kind)
        lib, ws, p, i64 = self.lib, self.ws, _lib.ptr, C.c_int64
        n_params = int(lib.ts_ppo_param_count(i64(obs_dim), i64(act_dim)))
        assert n_params == flat.numel()
        so = sigma_offset(obs_dim, act_dim)
        b = {k: t.to(device="cuda", dtype=torch.float32).contiguous() for k, t in batch.items()}
        perms = None if perms is None else [t.cuda() for t in perms]
        params, adam_m, adam_v = flat.cuda(), torch.zeros(n_params, device="cuda"), torch.zeros(n_params, device="cuda")
        grads = torch.zeros((STEPS, n_params), device="cuda")
        parts = torch.full((STEPS, 4), float("nan"), device="cuda")
        losses = torch.full((STEPS, 4), float("nan"), device="cuda")
        sigmas = torch.zeros((STEPS, act_dim), device="cuda")
        hp = P.PPOConfig(eps_clip=0.2, vf_coef=0.25, ent_coef=0.01, max_grad_norm=0.5, value_clip=True,
                         advantage_normalization=False, lr=3e-4).to_c()
        h_off = (C.c_int64 * 2)(0, rows)
        stream = _lib.current_stream(params.device)
        rec = torch.empty((rows, int(lib.ts_ppo_record_width(i64(obs_dim), i64(act_dim)))), device="cuda")
        with stepq_env(stepq):
            self.check(lib.ts_ppo_pack_batch(p(b["obs"]), p(b["act"]), p(b["adv"]), p(b["returns"]), p(b["logp_old"]), p(b["v_s"]),
                                             i64(rows), i64(obs_dim), i64(act_dim), p(rec), stream))
            for k in range(STEPS):
                perm = None if perms is None else perms[k]
                sigmas[k] = params[so:so + act_dim]
                self.check(lib.ts_ppo_invalidate_image(ws))            # ts_ppo_update moved the parameters under ts_ppo_grad's images
                self.check(lib.ts_ppo_grad(ws, p(params), i64(obs_dim), i64(act_dim), p(rec), i64(rows), p(perm), i64(rows), i64(rows),
                                           None, C.byref(hp), p(grads[k]), p(parts[k]), stream))
                self.check(lib.ts_ppo_update(ws, p(params), p(adam_m), p(adam_v), i64(k), i64(obs_dim), i64(act_dim), p(b["obs"]),
                                             p(b["act"]), p(b["adv"]), p(b["returns"]), p(b["logp_old"]), p(b["v_s"]), i64(rows),
                                             p(perm), h_off, i64(1), C.byref(hp), p(losses[k]) if with_losses else None, None,
                                             stream))
            torch.cuda.synchronize()
        return dict(gradient=grads, parts=parts, losses=losses, params=params, adam_m=adam_m, adam_v=adam_v, sigmas=sigmas)


@pytest.fixture(scope="module")
def branch():
    from tianshou_amd import _lib

    arm = Arm(_lib.load())
    cache = functools.lru_cache(maxsize=None)(arm.run)          # every case runs once, its results are shared and left unchanged
    yield arm, cache
    arm.close()


@pytest.fixture(scope="module")
def parent():
    path = os.environ.get("TS_PARENT_LIB")
    if not path:
        pytest.skip("TS_PARENT_LIB is not set: no libtsengine.so of the parent commit to compare bits with")
    from tianshou_amd import _lib

    _lib.load()                                                 # torch's HIP runtime first, as for the tree's own library
    arm = Arm(C.CDLL(path))
    yield arm
    arm.close()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", SLAB_CASES, ids=case_id)
def test_slab_counts_are_the_ones_meant(branch, case):
    arm, _ = branch
    with stepq_env(case[3]):
        assert arm.plan(*case[:3]) == (0, SLABS[case[2]])


def test_the_default_dispatch_case_runs_a_feature_split_kernel(branch):
    arm, _ = branch
    with stepq_env(STEPQ_CASE[3]):
        variant, slabs = arm.plan(*STEPQ_CASE[:3])
    assert variant in (1, 2) and slabs >= 1


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_entropy_of_both_paths(branch, case):
    _, run = branch
    out = run(case)
    assert torch.equal(bits(out["parts"][:, 3]), bits(out["losses"][:, 3]))
    ref = (0.5 + 0.5 * math.log(2.0 * math.pi) + out["sigmas"].double()).sum(dim=1).cpu().numpy()
    for name in ("parts", "losses"):
        got = out[name][:, 3].double().cpu().numpy()
        print(f"{case_id(case)} {name}[3]: max |diff| to float64 = {np.abs(got - ref).max():.3e}")
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
    assert bool(torch.isfinite(out["gradient"]).all()) and bool(out["gradient"].abs().sum() > 0)
    assert bool(torch.isfinite(out["losses"]).all()) and bool(torch.isfinite(out["parts"]).all())


@pytest.mark.parametrize("case", [SLAB_CASES[1], SLAB_CASES[3]], ids=case_id)
def test_update_without_losses_out_moves_the_same_state(branch, case):
    arm, run = branch
    with_l, without = run(case), arm.run(case, with_losses=False)
    for name in ("params", "adam_m", "adam_v"):
        assert torch.equal(bits(with_l[name]), bits(without[name])), name
    assert bool(torch.isnan(without["losses"]).all())          # nothing was written where no report was asked for


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bits_of_the_parent_commit(branch, parent, case):
    _, run = branch
    new, old = run(case), parent.run(case)
    for name in ("gradient", "parts", "losses", "params", "adam_m", "adam_v"):
        a, c = bits(new[name]), bits(old[name])
        assert torch.equal(a, c), f"{name}: {int((a != c).sum())} entries differ from the parent's"
