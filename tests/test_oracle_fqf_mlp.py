"""CPU: tests/oracle_fqf_mlp.py (the float64 reference of every FQF-MLP GPU test) and the stand-ins against the unmodified reference,
where it is mounted: three updates of the real FQF on the real FullQuantileFunction + FractionProposalNetwork over a Net, in both
feature forms and with both fraction optimizers, the oracle replaying the fractions the real network proposed.  Bars:
tests/test_oracle_iqn_mlp.py's."""
import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import oracle_fqf_mlp as OF
from tests import standin_fqf_mlp as SF


@pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference is not mounted")
@pytest.mark.parametrize("layers,freq,fopt", [((5, (64, 32), 64, 9, (32, 32, 32), 3), 2, "rmsprop"), ((5, (64, 32), 0, 64, (), 3), 0, "adam")])
def test_oracle_matches_the_reference(layers, freq, fopt):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.fqf import FQF, FQFPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory, RMSpropOptimizerFactory
    from tianshou.data import Batch, ReplayBuffer
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.discrete import FractionProposalNetwork, FullQuantileFunction

    obs_dim, trunk, feat, C, H, A = layers
    gamma, lr, ent, B, N = 0.9, 1e-3, 0.5, 24, 5
    torch.manual_seed(3)
    net = FullQuantileFunction(preprocess_net=Net(state_shape=obs_dim, action_shape=feat, hidden_sizes=list(trunk)), action_shape=A,
                               hidden_sizes=list(H), num_cosines=C)
    frac = FractionProposalNetwork(N, net.input_dim)
    with torch.no_grad():
        frac.net.weight.mul_(100.0)                            # (gain 0.01 leaves the proposal uniform to float32)
    mine, mine_frac = SF.build(layers, N)
    assert list(net.state_dict()) == list(mine.state_dict()) == list(OF.init_params(layers, 0))
    assert list(frac.state_dict()) == list(mine_frac.state_dict()) == list(OF.init_fraction_params(4, N, 0))
    algo = FQF(policy=FQFPolicy(model=net, fraction_model=frac, action_space=gym.spaces.Discrete(A)), optim=AdamOptimizerFactory(lr=lr),
               fraction_optim=(RMSpropOptimizerFactory if fopt == "rmsprop" else AdamOptimizerFactory)(lr=lr), gamma=gamma, num_fractions=N,
               ent_coef=ent, n_step_return_horizon=1, target_update_freq=freq)
    standin = SF.FQF(policy=SF.FQFPolicy(model=mine, fraction_model=mine_frac), ent_coef=ent, target_update_freq=freq)
    for name in ("ent_coef", "optim", "fraction_optim", "gamma", "n_step", "target_update_freq", "model_old", "_iter"):
        assert hasattr(algo, name) and hasattr(standin, name), name
    agent = OF.Agent(net.state_dict(), frac.state_dict(), layers, target_update_freq=freq, lr=lr, ent_coef=ent, f_optim=fopt, f_lr=lr)
    rng = np.random.default_rng(4)
    buf = ReplayBuffer(64)
    for t in range(60):
        term = bool(rng.random() < 0.2)
        buf.add(Batch(obs=rng.normal(size=obs_dim).astype(np.float32), act=int(rng.integers(A)), rew=float(rng.normal()), terminated=term,
                      truncated=False, obs_next=rng.normal(size=obs_dim).astype(np.float32), info={}))

    def proposed(obs):                                         # the fractions the real networks propose, float32
        with torch.no_grad():
            taus, tau_hats, ent_b = frac(net.preprocess(torch.as_tensor(obs))[0])
        for got, want in zip((taus, tau_hats, ent_b), agent.fractions(torch.as_tensor(obs))):
            np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=2e-6)
        return taus, tau_hats

    for u in range(3):
        idx = rng.integers(0, 60, B)
        batch = buf[idx]
        batch.weight = rng.uniform(0.3, 1.0, B)
        w = torch.as_tensor(batch.weight)
        algo.train()
        nd = agent.next_dist(torch.as_tensor(buf.obs_next[idx]), *proposed(buf.obs_next[idx]))
        batch = algo._preprocess_batch(batch, buf, idx)
        ret = torch.as_tensor(buf.rew[idx]).reshape(-1, 1) + gamma * nd * torch.as_tensor(1.0 - buf.terminated[idx]).reshape(-1, 1)
        np.testing.assert_allclose(np.asarray(batch.returns), ret.numpy(), rtol=1e-5, atol=2e-6)
        fractions = proposed(buf.obs[idx])
        stat = algo._update_with_batch(batch)
        losses, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), ret, w, *fractions)
        ql, fl, el = (float(x) for x in losses)
        for got, want in ((stat.quantile_loss, ql), (stat.fraction_loss, fl), (stat.entropy_loss, el), (stat.loss, ql + (fl - ent * el))):
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(batch.weight.detach().numpy(), prio.numpy(), rtol=1e-5, atol=2e-6)
        for mod, ref in ((net, agent.params), (frac, agent.fparams)):
            for k, p in mod.state_dict().items():
                np.testing.assert_allclose(p.numpy(), ref[k].detach().numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=k)
        if freq:
            for k, p in algo.model_old.module.state_dict().items():
                np.testing.assert_allclose(p.numpy(), agent.old[k].numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=k)
