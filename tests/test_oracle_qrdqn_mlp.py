"""CPU: tests/oracle_qrdqn_mlp.py (the float64 reference of every QRDQN-MLP GPU test) and the stand-in Net against the unmodified
reference, where it is mounted: three updates of the real QRDQN on the real Net(num_atoms=N).  Bars: tests/test_oracle_dqn_mlp.py's."""
import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import oracle_qrdqn_mlp as OQ
from tests import standin_qrdqn_mlp as SQ

LAYERS = (5, (64, 32), 3, 7)


@pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference is not mounted")
@pytest.mark.parametrize("freq", [2, 0])
def test_oracle_matches_the_reference(freq):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.qrdqn import QRDQN, QRDQNPolicy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import Batch, ReplayBuffer
    from tianshou.utils.net.common import Net

    obs_dim, trunk, A, N = LAYERS
    torch.manual_seed(3)
    net = Net(state_shape=obs_dim, action_shape=A, hidden_sizes=list(trunk), softmax=False, num_atoms=N)
    mine = SQ.build(LAYERS)
    assert list(net.state_dict()) == list(mine.state_dict()) == list(OQ.init_params(LAYERS, 0))
    mine.load_state_dict(net.state_dict())
    x = torch.randn(4, obs_dim)
    assert torch.equal(net(x)[0], mine(x)[0].view(4, A, N))
    np.testing.assert_allclose(net(x)[0].detach().numpy(), OQ.forward(net.state_dict(), LAYERS, x).numpy(), rtol=1e-5, atol=2e-6)
    gamma, lr, B = 0.9, 1e-3, 24
    algo = QRDQN(policy=QRDQNPolicy(model=net, action_space=gym.spaces.Discrete(A)), optim=AdamOptimizerFactory(lr=lr), gamma=gamma,
                 num_quantiles=N, n_step_return_horizon=1, target_update_freq=freq)
    agent = OQ.Agent(net.state_dict(), LAYERS, target_update_freq=freq, lr=lr)
    assert torch.equal(agent.tau_hat, algo.tau_hat.data)
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
        td = agent.target_dist(torch.as_tensor(buf.obs_next[idx]))
        ret = torch.as_tensor(buf.rew[idx]).reshape(-1, 1) + gamma * td * torch.as_tensor(1.0 - buf.terminated[idx]).reshape(-1, 1)
        np.testing.assert_allclose(np.asarray(batch.returns), ret.numpy(), rtol=1e-5, atol=2e-6)
        algo.train()
        stat = algo._update_with_batch(batch)
        loss, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), ret, w)
        np.testing.assert_allclose(stat.loss, float(loss), rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(batch.weight.detach().numpy(), prio.numpy(), rtol=1e-5, atol=2e-6)
        for k, p in net.state_dict().items():
            np.testing.assert_allclose(p.numpy(), agent.params[k].numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=k)
            if freq:
                np.testing.assert_allclose(algo.model_old.module.state_dict()[k].numpy(), agent.old[k].numpy(), rtol=1e-5, atol=0.02 * lr, err_msg=k)
