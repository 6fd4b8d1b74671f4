"""GPU parity of the step kernel's RAW gradient (before clip + Adam, which normalise away a mis-scaled block) for every
first-layer width class of the dW1 phase: KP = 2 KS1 = 2, 8, 16 (one 16-column tile), 18 (two columns in the second
tile; obs 16 leaves one of them a zero column), 24 and 32 (two tiles), with 1, 6 and 8 actions, on one partial
tile, one full workgroup and a second workgroup with a single live wave, with and without a row permutation; the slab
accumulation of a second grid pass on both dW1 paths; and the one-network kernel, which shares the weight-gradient code.
Reference: autograd of oracle_ppo.ppo_minibatch_loss (torch fp32 on the CPU).  Bars: losses rtol 1e-5, every parameter
block within 1e-5 of the block's largest entry (test_gpu_ppo.assert_blocks_close)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_ppo as OP

from tests.test_gpu_ppo import assert_blocks_close, dev, random_problem

pytestmark = pytest.mark.gpu

KW = dict(eps_clip=0.2, value_clip=True, advantage_normalization=True, vf_coef=0.25, ent_coef=0.01,
          max_grad_norm=0.5, lr=3e-4)


@functools.lru_cache(maxsize=4)
def problem(n, obs_dim, act_dim):
    """Inputs of one minibatch step over all n rows and the reference losses / gradient (computed once per shape: a row
    permutation only reorders the sum).  The returns sit 0.5 above the critic's values on average: c_bv is a block of ONE
    entry, the mean of the value-loss derivatives, and around a zero-mean target it cancels to ~1 / sqrt(n) of its terms --
    at 70,036 rows to 1e-4, where the 1e-5 bar of a block's own scale would measure the rounding of a sum of O(1) terms
    against a number that is small by accident."""
    params, data = random_problem(n, obs_dim, act_dim, seed=1000 * obs_dim + 10 * act_dim + n % 7)
    obs, act = torch.from_numpy(data["obs"]), torch.from_numpy(data["act"])
    rng = np.random.default_rng(n + obs_dim)
    with torch.no_grad():
        v = OP.critic_forward(params, obs).flatten()
        mu, sigma = OP.actor_forward(params, obs)
        logp = OP.dist_of(mu, sigma).log_prob(act)
    b = dict(obs=obs, act=act,
             adv=torch.from_numpy(rng.normal(size=n).astype(np.float32)),
             returns=v + 0.5 + torch.from_numpy(rng.normal(size=n).astype(np.float32)),
             logp_old=logp + torch.from_numpy(rng.normal(scale=0.3, size=n).astype(np.float32)),
             v_s=v + torch.from_numpy(rng.normal(scale=0.2, size=n).astype(np.float32)))
    torch.set_num_threads(8)
    p = {k: t.clone().requires_grad_(True) for k, t in params.items()}
    losses = OP.ppo_minibatch_loss(p, OP.PPOConfig(**KW), obs, act, b["adv"], b["returns"], b["logp_old"], b["v_s"])
    losses[0].backward()
    g_ref = torch.cat([p[k].grad.reshape(-1) for k in OP.PARAM_ORDER]).numpy()
    return params, b, [x.item() for x in losses], g_ref


def run_step(n, obs_dim, act_dim, permuted, nets=0):
    from tianshou_amd import ppo as P

    params, b, losses_ref, g_ref = problem(n, obs_dim, act_dim)
    eng = P.PPOEngine(obs_dim, act_dim, OP.flatten_params(params).cuda(), P.PPOConfig(nets=nets, **KW))
    perm = dev(np.random.default_rng(n).permutation(n)) if permuted else None
    losses, grads = eng._run_steps({k: t.cuda() for k, t in b.items()}, perm, [0, n], want_grad=True)
    return losses.cpu().numpy()[0], grads.cpu().numpy(), losses_ref, g_ref


SHAPES = [(o, 6) for o in (1, 7, 15, 16, 17, 23, 31)] + [(17, 1), (17, 8)]


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("n", [31, 128, 160])
@pytest.mark.parametrize("obs_dim,act_dim", SHAPES)
def test_raw_gradient_every_width_class(obs_dim, act_dim, n, permuted):
    losses, grads, losses_ref, g_ref = run_step(n, obs_dim, act_dim, permuted)
    np.testing.assert_allclose(losses, losses_ref, rtol=1e-5, atol=1e-6)
    assert_blocks_close(grads, g_ref, obs_dim, act_dim)


@pytest.mark.parametrize("obs_dim", [15, 31])
def test_raw_gradient_second_grid_pass(obs_dim):
    """More rows than 512 workgroups x 128: the slab accumulation (`first == false`) of the one-tile and the two-tile path."""
    losses, grads, losses_ref, g_ref = run_step(65536 + 4500, obs_dim, 6, True)
    np.testing.assert_allclose(losses, losses_ref, rtol=1e-5, atol=1e-6)
    assert_blocks_close(grads, g_ref, obs_dim, 6)


@pytest.mark.parametrize("nets", [1, 2])
def test_raw_gradient_one_network_kernel(nets):
    """ppo_step1_kernel (nets = 1: actor, 2: critic) on 160 rows at obs 17: the live network's blocks against autograd,
    the absent network's exactly zero."""
    from tianshou_amd import ppo as P

    obs_dim, act_dim = 17, 6
    losses, grads, losses_ref, g_ref = run_step(160, obs_dim, act_dim, True, nets=nets)
    shapes = P.param_shapes(obs_dim, act_dim)
    n_actor = sum(int(np.prod(shapes[k])) for k in P.PARAM_ORDER[:7])
    dead = slice(n_actor, None) if nets == 1 else slice(0, n_actor)
    assert not grads[dead].any()
    np.testing.assert_allclose(losses[nets], losses_ref[nets], rtol=1e-5, atol=1e-6)      # clip loss / value loss
    filled = grads.copy()
    filled[dead] = g_ref[dead]                     # the dead blocks were checked above: let the block bar see the live ones
    assert_blocks_close(filled, g_ref, obs_dim, act_dim)
