"""CPU: tests/oracle_iqn_mlp.py (the float64 reference of every IQN-MLP GPU test) and the stand-ins against the unmodified reference,
where it is mounted: three updates of the real IQN on the real ImplicitQuantileNetwork over a Net, in both feature forms, the oracle
replaying the fractions the real network drew.  Bars: tests/test_oracle_qrdqn_mlp.py's."""
import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import oracle_iqn_mlp as OI
from tests import standin_iqn_mlp as SI


@pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference is not mounted")
@pytest.mark.parametrize("layers,freq", [((5, (64, 32), 64, 9, (32,), 3), 2), ((5, (64, 32), 0, 64, (), 3), 0)])
def test_oracle_matches_the_reference(layers, freq):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.iqn import IQN, IQNPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import Batch, ReplayBuffer
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.discrete import ImplicitQuantileNetwork

    obs_dim, trunk, feat, C, H, A = layers
    torch.manual_seed(3)
    net = ImplicitQuantileNetwork(preprocess_net=Net(state_shape=obs_dim, action_shape=feat, hidden_sizes=list(trunk)), action_shape=A,
                                  hidden_sizes=list(H), num_cosines=C)
    mine = SI.build(layers)
    assert list(net.state_dict()) == list(mine.state_dict()) == list(OI.init_params(layers, 0))
    drawn, rand = [], torch.rand
    torch.rand = lambda *a, **k: (drawn.append(rand(*a, **k)), drawn[-1])[1]          # the fractions the real network draws
    try:
        gamma, lr, B, N, N2 = 0.9, 1e-3, 24, 5, 7
        algo = IQN(policy=IQNPolicy(model=net, action_space=gym.spaces.Discrete(A), sample_size=4, online_sample_size=N, target_sample_size=N2),
                   optim=AdamOptimizerFactory(lr=lr), gamma=gamma, n_step_return_horizon=1, target_update_freq=freq)
        agent = OI.Agent(net.state_dict(), layers, target_update_freq=freq, lr=lr)
        rng = np.random.default_rng(4)
        buf = ReplayBuffer(64)
        for t in range(60):
            term = bool(rng.random() < 0.2)
            buf.add(Batch(obs=rng.normal(size=obs_dim).astype(np.float32), act=int(rng.integers(A)), rew=float(rng.normal()), terminated=term,
                          truncated=False, obs_next=rng.normal(size=obs_dim).astype(np.float32), info={}))
        for u in range(3):
            idx = rng.integers(0, 60, B)
            batch = buf[idx]
            batch.weight = rng.uniform(0.3, 1.0, B)
            w = torch.as_tensor(batch.weight)
            del drawn[:]
            algo.train()
            batch = algo._preprocess_batch(batch, buf, idx)
            assert [tuple(t.shape) for t in drawn] == ([(B, N), (B, N2)] if freq else [(B, N)])       # online fractions first
            nd = agent.next_dist(torch.as_tensor(buf.obs_next[idx]), drawn[0], drawn[1] if freq else None)
            ret = torch.as_tensor(buf.rew[idx]).reshape(-1, 1) + gamma * nd * torch.as_tensor(1.0 - buf.terminated[idx]).reshape(-1, 1)
            np.testing.assert_allclose(np.asarray(batch.returns), ret.numpy(), rtol=1e-5, atol=2e-6)
            del drawn[:]
            stat = algo._update_with_batch(batch)
            loss, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), ret, w, drawn[0])
            np.testing.assert_allclose(stat.loss, float(loss), rtol=1e-5, atol=2e-6)
            np.testing.assert_allclose(batch.weight.detach().numpy(), prio.numpy(), rtol=1e-5, atol=2e-6)
            for k, p in net.state_dict().items():
                np.testing.assert_allclose(p.numpy(), agent.params[k].numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=k)
                if freq:
                    np.testing.assert_allclose(algo.model_old.module.state_dict()[k].numpy(), agent.old[k].numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=k)
    finally:
        torch.rand = rand
