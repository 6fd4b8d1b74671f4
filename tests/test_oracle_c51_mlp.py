"""CPU: tests/oracle_c51_mlp.py and the stand-in Net against the unmodified reference, where it is mounted: three updates of the real C51 on the
real Net(softmax=True, num_atoms=N) in float64 arithmetic (bars 1e-7: the reference keeps returns and importance weights as float32 tensors)."""
import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import oracle_c51_mlp as OC
from tests import standin_c51_mlp as SC

LAYERS = (5, (64, 32), 3, 7)


@pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference is not mounted")
@pytest.mark.parametrize("freq", [2, 0])
def test_oracle_matches_the_reference(freq):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.c51 import C51, C51Policy
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import Batch, ReplayBuffer
    from tianshou.utils.net.common import Net

    obs_dim, trunk, A, N = LAYERS
    torch.manual_seed(3)
    net = Net(state_shape=obs_dim, action_shape=A, hidden_sizes=list(trunk), softmax=True, num_atoms=N)
    assert list(net.state_dict()) == list(SC.build(LAYERS).state_dict()) == list(OC.init_params(LAYERS, 0))
    gamma, lr, B, v_min, v_max = 0.9, 1e-3, 24, -2.0, 2.0
    agent = OC.Agent(net.state_dict(), LAYERS, target_update_freq=freq, lr=lr, v_min=v_min, v_max=v_max)
    net = net.double()                                                        # MLP.forward casts obs to float32 (common.py:175):
    net.model.model[0].register_forward_pre_hook(lambda m, a: (a[0].double(),))   # float32 observations, float64 from there on
    x = torch.randn(4, obs_dim)
    np.testing.assert_allclose(net(x)[0].detach().numpy(), OC.forward(agent.params, LAYERS, x).numpy(), rtol=1e-12, atol=1e-14)
    algo = C51(policy=C51Policy(model=net, action_space=gym.spaces.Discrete(A), num_atoms=N, v_min=v_min, v_max=v_max),
               optim=AdamOptimizerFactory(lr=lr), gamma=gamma, n_step_return_horizon=1, target_update_freq=freq)
    assert torch.equal(agent.support, algo.policy.support.data) and agent.delta_z == algo.delta_z
    rng = np.random.default_rng(4)
    buf = ReplayBuffer(64)
    for t in range(60):
        term = bool(rng.random() < 0.2)
        buf.add(Batch(obs=rng.normal(size=obs_dim).astype(np.float32), act=int(rng.integers(A)), rew=float(2 * rng.normal()), terminated=term,
                      truncated=False, obs_next=rng.normal(size=obs_dim).astype(np.float32), info={}))
    for u in range(3):
        idx = rng.integers(0, 60, B)
        batch = buf[idx]
        batch.weight = rng.uniform(0.3, 1.0, B)
        w = torch.as_tensor(batch.weight)
        batch = algo._preprocess_batch(batch, buf, idx)
        ret = torch.as_tensor(buf.rew[idx]).reshape(-1, 1) + gamma * agent.support.double() * torch.as_tensor(1.0 - buf.terminated[idx]).reshape(-1, 1)
        np.testing.assert_allclose(np.asarray(batch.returns), ret.numpy(), rtol=1e-5, atol=2e-6)
        ret = torch.as_tensor(np.asarray(batch.returns))
        assert float(ret.min()) < v_min and float(ret.max()) > v_max           # the clamp is exercised
        algo.train()
        stat = algo._update_with_batch(batch)
        loss, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), torch.as_tensor(buf.obs_next[idx]), ret, w)
        np.testing.assert_allclose(stat.loss, float(loss), rtol=1e-7)
        np.testing.assert_allclose(batch.weight.detach().numpy(), prio.numpy(), rtol=1e-7, atol=1e-12)
        for k, p in net.state_dict().items():
            np.testing.assert_allclose(p.numpy(), agent.params[k].numpy(), rtol=1e-7, atol=1e-9, err_msg=k)
            if freq:
                np.testing.assert_allclose(algo.model_old.module.state_dict()[k].numpy(), agent.old[k].numpy(), rtol=1e-7, atol=1e-9, err_msg=k)
