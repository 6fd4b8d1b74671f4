"""CPU: tests/oracle_rainbow_mlp.py and the stand-in Net against the unmodified reference, where it is mounted: three updates of the real RainbowDQN on
the real Net with NoisyLinear streams in float64 arithmetic (bars 1e-7, as tests/test_oracle_c51_mlp.py: returns and importance weights stay float32)."""
import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import oracle_rainbow_mlp as OR
from tests import standin_rainbow_mlp as SR

LAYERS = (5, (64, 32), (32,), (), 3, 7, True)


@pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference is not mounted")
@pytest.mark.parametrize("freq", [2, 0])
def test_oracle_matches_the_reference(freq):
    ref_shim.install()
    import gymnasium as gym
    from tianshou.algorithm.modelfree.c51 import C51Policy
    from tianshou.algorithm.modelfree.rainbow import RainbowDQN
    from tianshou.algorithm.optim import AdamOptimizerFactory
    from tianshou.data import Batch, ReplayBuffer
    from tianshou.utils.net.common import ModuleWithVectorOutput, Net
    from tianshou.utils.net.discrete import NoisyLinear

    obs_dim, trunk, qh, vh, A, N, _ = LAYERS
    torch.manual_seed(3)
    noisy = lambda x, y: NoisyLinear(x, y, 0.5)  # noqa: E731
    net = Net(state_shape=obs_dim, action_shape=A, hidden_sizes=list(trunk), softmax=True, num_atoms=N,
              dueling_param=({"linear_layer": noisy, "hidden_sizes": list(qh)}, {"linear_layer": noisy, "hidden_sizes": list(vh)}))
    keys = [k for k, p in net.named_parameters() if p.requires_grad]
    assert list(net.state_dict()) == list(SR.build(LAYERS).state_dict()) and keys == list(OR.init_params(LAYERS, 0))
    gamma, lr, B, v_min, v_max = 0.9, 1e-3, 24, -2.0, 2.0
    agent = OR.Agent({k: net.state_dict()[k] for k in keys}, LAYERS, None, target_update_freq=freq, lr=lr, v_min=v_min, v_max=v_max)
    net = net.double()                                                        # MLP.forward casts its input to float32 (common.py:175):
    net.model.model[0].register_forward_pre_hook(lambda m, a: (a[0].double(),))   # float32 observations, float64 from there on, so the
    net.Q, net.V = (ModuleWithVectorOutput.from_module(m.model, m.output_dim) for m in (net.Q, net.V))   # streams run without that cast
    name = lambda k: k.replace(".module.", ".model.")  # noqa: E731
    eps_of = lambda mod: {name(k): p.detach().clone() for k, p in mod.state_dict().items() if "eps_" in k}  # noqa: E731
    algo = RainbowDQN(policy=C51Policy(model=net, action_space=gym.spaces.Discrete(A), num_atoms=N, v_min=v_min, v_max=v_max),
                      optim=AdamOptimizerFactory(lr=lr), gamma=gamma, n_step_return_horizon=1, target_update_freq=freq)
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
        ret = torch.as_tensor(np.asarray(batch.returns))
        algo.train()
        state = torch.get_rng_state()                                          # the noise _update_with_batch is about to draw
        algo._sample_noise(net)
        if freq:
            algo._sample_noise(algo.model_old)
        agent.noise, agent.noise_old = eps_of(net), eps_of(algo.model_old) if freq else None
        torch.set_rng_state(state)
        stat = algo._update_with_batch(batch)
        loss, prio = agent.update(torch.as_tensor(buf.obs[idx]), torch.as_tensor(buf.act[idx]), torch.as_tensor(buf.obs_next[idx]), ret, w)
        np.testing.assert_allclose(stat.loss, float(loss), rtol=1e-7)
        np.testing.assert_allclose(batch.weight.detach().numpy(), prio.numpy(), rtol=1e-7, atol=1e-12)
        for k, p in net.state_dict().items():
            if "eps_" in k:
                continue
            np.testing.assert_allclose(p.numpy(), agent.params[name(k)].numpy(), rtol=1e-7, atol=1e-9, err_msg=k)
            if freq:
                np.testing.assert_allclose(algo.model_old.state_dict()[k].numpy(), agent.old[name(k)].numpy(), rtol=1e-7, atol=1e-9, err_msg=k)
