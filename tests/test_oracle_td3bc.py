"""CPU: tests/oracle_td3bc.py (the torch restatement the GPU parity tests compare against) replays the fixtures recorded from
the UNMODIFIED reference TD3BC.update() (tools/gen_golden_td3bc.py) at the bars tests/test_oracle_golden.py uses for the td3_*
fixtures; where the reference is mounted, the generator reproduces both files bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import oracle_sac as OS
from oracle import ref_shim
from tests import oracle_td3bc as OB
from tests import td3bc_common as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", CC.TAGS)
def test_td3bc_restatement_matches_reference(tag):
    """Returns, statistics and strided networks at test_td3_ddpg_restatement_matches_reference's bars (returns rtol 1e-5 /
    atol 1e-5, statistics rtol 1e-5 / atol 1e-7, networks rtol 1e-5 / atol 1e-6).  What the td3_* fixtures do not hold:
    the new priorities (td1 + td2) / 2 at the returns' bar, of which they are differences; the PER draw, weights and sum-tree
    as tests/test_oracle_dcql.py replays them (exact indices, rtol 1e-4); the final Adam moments at that test's bars (first
    moments rtol 1e-5 / atol 1e-8, second moments rtol 1e-5 / atol 1e-12)."""
    g, d, cfg, bstate = CC.load_td3bc(tag)
    st = OS.TD3State.create(*OS.init_td3_params(d["obs_dim"], d["act_dim"], d["seed"], True, d["hidden"]), cfg)
    obs_all, obs_next_all = torch.as_tensor(g["obs"]), torch.as_tensor(g["obs_next"])
    if d["prioritized"]:
        tree = g["tree0"].copy()
        bound = 1
        while bound < d["E"] * d["slots"]:
            bound *= 2
        np.random.seed(d["seed"] + 7)
        mx, mn = 1.0, 1.0
    else:
        assert not any(k.endswith("is_weight") or k.endswith("tree") for k in g.files)
    with OS.activation(d["activation"]):
        for u in range(d["n_updates"]):
            idx, noise = g[f"u{u}_indices"], g[f"u{u}_noise"]
            w = None
            if d["prioritized"]:
                scalar = np.random.rand(d["batch"]) * tree[1]
                assert np.array_equal(O._get_prefix_sum_idx(scalar, bound, tree), idx)
                w = O.per_get_weight(tree, bound, idx, mn, 0.4, True)
                np.testing.assert_allclose(w, g[f"u{u}_is_weight"], rtol=1e-4)
            ret, _ = O.compute_nstep_return(bstate, idx, lambda after: OS.td3_target_q(st, cfg, obs_next_all[after], noise).numpy(),
                                            cfg.gamma, cfg.n_step)
            ret = ret.astype(np.float32).reshape(-1)
            np.testing.assert_allclose(ret, g[f"u{u}_returns"], rtol=1e-5, atol=1e-5)
            out = OB.update_with_batch(st, cfg, obs_all[idx], g["act"][idx], ret, weight=w)
            np.testing.assert_allclose([out["actor_loss"], out["critic1_loss"], out["critic2_loss"]], g[f"u{u}_stats"], rtol=1e-5,
                                       atol=1e-7)
            np.testing.assert_allclose(out["weight"].numpy(), g[f"u{u}_prio"], rtol=1e-5, atol=1e-5)
            for name in CC.NETS:
                order = OS.order_of(getattr(st, name))
                np.testing.assert_allclose(OS.flatten(getattr(st, name), order).numpy()[::61], g[f"u{u}_{name}"], rtol=1e-5,
                                           atol=1e-6, err_msg=name)
            if d["prioritized"]:
                mx, mn = O.per_update_weight(tree, bound, idx, out["weight"].numpy(), 0.6, mx, mn)
                np.testing.assert_allclose(tree, g[f"u{u}_tree"], rtol=1e-4)
    assert st.cnt == d["n_updates"]
    for name, opt in (("actor", st.opt_actor), ("critic1", st.opt_c1), ("critic2", st.opt_c2)):
        assert opt.step == int(g[f"adam_step_{name}"]), name
        order = OS.order_of(getattr(st, name))
        np.testing.assert_allclose(OS.flatten(opt.m, order).numpy()[::61], g[f"adam_m_{name}"], rtol=1e-5, atol=1e-8, err_msg=name)
        np.testing.assert_allclose(OS.flatten(opt.v, order).numpy()[::61], g[f"adam_v_{name}"], rtol=1e-5, atol=1e-12, err_msg=name)


def test_fixtures_are_the_two_the_issue_describes():
    g, d, cfg, _ = CC.load_td3bc("offline")
    assert (d["obs_dim"], d["act_dim"], d["batch"], d["n_updates"], d["prioritized"], d["activation"]) == (23, 5, 64, 4, False, "relu")
    assert d["hidden"] == ((256, 256), (256, 256)) and (cfg.alpha, cfg.update_actor_freq, cfg.n_step) == (2.5, 2, 1)
    assert int(g["adam_step_actor"]) == 2 and int(g["adam_step_critic1"]) == 4          # two actor steps in four updates
    g, d, cfg, _ = CC.load_td3bc("per_tanh")
    assert (d["n_updates"], d["prioritized"], d["activation"]) == (3, True, "tanh")
    sa, sc = d["hidden"]
    assert len(sa) == len(sc) == 3 and len(set(sa)) == 3 and len(set(sc)) == 3 and sa != sc
    assert (cfg.alpha, cfg.update_actor_freq, cfg.n_step, cfg.max_action) == (1.0, 1, 3, 1.5)
    biggest = max(os.path.getsize(os.path.join(CC.GOLDEN, f)) for f in os.listdir(CC.GOLDEN) if f.startswith("td3_"))
    for tag in CC.TAGS:
        assert os.path.getsize(os.path.join(CC.GOLDEN, f"td3bc_{tag}.npz")) <= biggest


def test_actor_term_of_the_restatement_against_float64_closed_form():
    """oracle_td3bc.actor_loss_terms on a small net: lmbda, the loss and its gradient w.r.t. the head bias equal the closed form
    d/d head = (lmbda * dQ/da * (-1/B) + 2 (a - a_data) / (B A)) * max_action * (1 - tanh^2), evaluated in float64."""
    obs_dim, A, B, max_action, alpha = 7, 3, 9, 1.5, 2.5
    actor, c1, _ = OS.init_td3_params(obs_dim, A, 5, True, 64)
    g = torch.Generator().manual_seed(1)
    obs, act = torch.randn(B, obs_dim, generator=g), torch.rand(B, A, generator=g) * 3 - 1.5
    p = {k: v.clone().requires_grad_(True) for k, v in actor.items()}
    loss, lmbda, q, pi = OB.actor_loss_terms(p, c1, obs, act, max_action, alpha)
    got = torch.autograd.grad(loss, p["ba"])[0].double()
    a64, c64 = {k: v.double() for k, v in actor.items()}, {k: v.double() for k, v in c1.items()}
    head = torch.nn.functional.linear(OS.trunk_forward(a64, obs.double()), a64["wa"], a64["ba"])
    t = torch.tanh(head)
    a = (max_action * t).requires_grad_(True)
    q64 = OS.critic_forward(c64, obs.double(), a).flatten()
    dq_da = torch.autograd.grad(q64.sum(), a)[0]
    lm64 = alpha / q64.abs().mean().detach()
    want_loss = -lm64 * q64.mean() + ((a - act.double()) ** 2).mean()
    d_head = (-lm64 * dq_da / B + 2.0 * (a.detach() - act.double()) / (B * A)) * max_action * (1.0 - t * t)
    assert abs(float(lmbda.detach()) - float(lm64)) <= 1e-5 * float(lm64)
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-5 * abs(float(want_loss))
    assert float((got - d_head.sum(0)).abs().max()) <= 1e-5 * float(d_head.sum(0).abs().max())


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference not mounted")
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, TS_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="random")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_td3bc.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for tag in CC.TAGS:
        f = f"td3bc_{tag}.npz"
        new, old = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(CC.GOLDEN, f))
        assert sorted(new.files) == sorted(old.files), f
        same = lambda a, b: np.array_equal(a, b, equal_nan=a.dtype.kind == "f")      # noqa: E731 (string arrays: no isnan)
        bad = [k for k in old.files if not same(new[k], old[k])]
        assert not bad, (f, bad[:5])
