"""Minimal stand-in of the reference's TD3BC class for the GPU tests (the reference package is absent on the GPU box), on top
of tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_td3bc` touches and nothing else.
test_td3bc_shim.py checks it against the real class where the reference is mounted."""
from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_td3bc(ref=...) resolves every name in one namespace)


class TD3BC(SI.TD3):
    """imitation/td3_bc.py:14-100: TD3's attributes plus `alpha`; without a second critic the first one is copied
    (td3.py:90)."""

    def __init__(self, *, policy, critic, critic2=None, lr=1e-3, critic_lr=None, tau=0.005, gamma=0.99, policy_noise=0.2,
                 update_actor_freq=2, noise_clip=0.5, alpha=2.5, n_step_return_horizon=1):
        import copy

        super().__init__(policy=policy, critic=critic, critic2=critic2 if critic2 is not None else copy.deepcopy(critic), lr=lr,
                         critic_lr=critic_lr, tau=tau, gamma=gamma, policy_noise=policy_noise, update_actor_freq=update_actor_freq,
                         noise_clip=noise_clip, n_step_return_horizon=n_step_return_horizon)
        self.alpha = alpha
