"""CPU: tests/oracle_dqn_mlp.py (the float64 reference of every DQN-MLP GPU test) and the stand-in Net against the unmodified
reference, where it is mounted: three updates of the real DQN on the real dueling Net."""
import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import oracle_dqn_mlp as OM
from tests import standin_dqn_mlp as SM

LAYERS = (5, (64, 32), (32,), (64, 32), 3)


@pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference is not mounted")
@pytest.mark.parametrize("huber,double", [(None, True), (0.7, False)])
def test_oracle_matches_the_reference(huber, double):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.dqn import DQN, DiscreteQLearningPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import Batch, ReplayBuffer
    from tianshou.utils.net.common import Net

    obs_dim, trunk, q, v, A = LAYERS
    torch.manual_seed(3)
    net = Net(state_shape=obs_dim, action_shape=A, hidden_sizes=list(trunk), dueling_param=({"hidden_sizes": list(q)}, {"hidden_sizes": list(v)}))
    mine = SM.build(LAYERS)
    assert list(net.state_dict()) == list(mine.state_dict()) == list(OM.shapes(LAYERS))
    assert {k: tuple(p.shape) for k, p in net.state_dict().items()} == OM.shapes(LAYERS)
    mine.load_state_dict(net.state_dict())
    x = torch.randn(4, obs_dim)
    assert torch.equal(net(x)[0], mine(x)[0])
    gamma, lr, B = 0.9, 1e-3, 24
    algo = DQN(policy=DiscreteQLearningPolicy(model=net, action_space=gym.spaces.Discrete(A)), optim=AdamOptimizerFactory(lr=lr), gamma=gamma,
               n_step_return_horizon=1, target_update_freq=2, is_double=double, huber_loss_delta=huber)
    agent = OM.Agent(net.state_dict(), LAYERS, target_update_freq=2, is_double=double, huber_delta=huber, lr=lr)
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
        batch = algo._preprocess_batch(batch, buf, idx)
        tq = agent.target_q(torch.as_tensor(buf.obs_next[idx]))
        ret = torch.as_tensor(buf.rew[idx]) + gamma * tq * torch.as_tensor(1.0 - buf.terminated[idx])
        np.testing.assert_allclose(np.asarray(batch.returns).reshape(-1), ret.numpy(), rtol=1e-5, atol=2e-6)
        algo.train()
        stat = algo._update_with_batch(batch)
        loss, td = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), ret, w)
        np.testing.assert_allclose(stat.loss, float(loss), rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(batch.weight.detach().numpy(), td.numpy(), rtol=1e-5, atol=2e-6)
        for k, p in net.state_dict().items():
            np.testing.assert_allclose(p.numpy(), agent.params[k].numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=k)
            np.testing.assert_allclose(algo.model_old.module.state_dict()[k].numpy(), agent.old[k].numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=k)
