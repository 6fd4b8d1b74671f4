"""Minimal stand-ins of the reference's continuous BCQ classes for the GPU tests (the reference package is absent on the GPU
box), on top of tests/standin.py: the attribute surface `tianshou_amd.integration.make_hip_bcq` touches and nothing else.
tests/test_cbcq_shim.py checks them against the real classes where the reference is mounted."""
import copy
from dataclasses import dataclass

from torch import nn

from tests import standin as SI
from tests.standin import *  # noqa: F401,F403  (make_hip_bcq(ref=...) resolves every name in one namespace)


@dataclass(kw_only=True)
class BCQTrainingStats:
    """imitation/bcq.py:23-28."""

    actor_loss: float
    critic1_loss: float
    critic2_loss: float
    vae_loss: float
    train_time: float = 0.0


class MLP(SI._MLP):
    """utils/net/common.py:90-178: MLP(input_dim, output_dim, hidden_sizes): the activation after every hidden Linear, a last
    Linear without one when output_dim > 0.  `forward` returns a tensor (no state)."""

    def __init__(self, *, input_dim, output_dim=0, hidden_sizes=(), activation=nn.ReLU):
        super().__init__([input_dim, *hidden_sizes], activation)
        if output_dim > 0:
            self.model.append(nn.Linear(hidden_sizes[-1] if hidden_sizes else input_dim, output_dim))
        self.output_dim = output_dim or hidden_sizes[-1]


class Net(nn.Module):
    """`Net(state_shape, action_shape, hidden_sizes)` (utils/net/common.py:246-369): `.model` is an MLP -- with an output layer
    of `out_dim` when it is given (no concat), without one for a critic's trunk (concat=True); `forward` returns (logits, state)."""

    def __init__(self, in_dim, hidden_sizes, activation=nn.ReLU, out_dim=0):
        super().__init__()
        self.model = MLP(input_dim=in_dim, output_dim=out_dim, hidden_sizes=hidden_sizes, activation=activation)
        self.output_dim = out_dim or hidden_sizes[-1]


class Perturbation(nn.Module):
    """utils/net/continuous.py:378-412."""

    def __init__(self, *, preprocess_net, max_action, phi=0.05):
        super().__init__()
        self.preprocess_net, self.max_action, self.phi = preprocess_net, max_action, phi


class VAE(nn.Module):
    """utils/net/continuous.py:415-490."""

    def __init__(self, *, encoder, decoder, hidden_dim, latent_dim, max_action):
        super().__init__()
        self.encoder = encoder
        self.mean, self.log_std = nn.Linear(hidden_dim, latent_dim), nn.Linear(hidden_dim, latent_dim)
        self.decoder = decoder
        self.max_action, self.latent_dim = max_action, latent_dim


class BCQPolicy(nn.Module):
    """imitation/bcq.py:34-116."""

    def __init__(self, *, actor_perturbation, critic, vae, forward_sampled_times=100, action_space=None):
        super().__init__()
        self.actor_perturbation, self.critic, self.vae = actor_perturbation, critic, vae
        self.forward_sampled_times, self.action_space = forward_sampled_times, action_space
        self.is_within_training_step = False


class BCQ(SI.Algorithm):
    """imitation/bcq.py:119-186: the four optimizers and three lagged networks under the reference's names."""

    def __init__(self, *, policy, critic2=None, actor_perturbation_lr=1e-3, critic_lr=1e-3, critic2_lr=None, vae_lr=1e-3, gamma=0.99,
                 tau=0.005, lmbda=0.75, num_sampled_action=10):
        super().__init__(policy)
        self.tau = tau
        self.actor_perturbation_target = SI.EvalModeModuleWrapper(copy.deepcopy(policy.actor_perturbation))
        self.actor_perturbation_optim = self._create_optimizer(policy.actor_perturbation, actor_perturbation_lr)
        self.critic_target = SI.EvalModeModuleWrapper(copy.deepcopy(policy.critic))
        self.critic_optim = self._create_optimizer(policy.critic, critic_lr)
        self.critic2 = critic2 or copy.deepcopy(policy.critic)
        self.critic2_target = SI.EvalModeModuleWrapper(copy.deepcopy(self.critic2))
        self.critic2_optim = self._create_optimizer(self.critic2, critic2_lr or critic_lr)
        self.vae_optim = self._create_optimizer(policy.vae, vae_lr)
        self.gamma, self.lmbda, self.num_sampled_action = gamma, lmbda, num_sampled_action

    def _preprocess_batch(self, batch, buffer, indices):
        return batch

    def update(self, buffer, sample_size):
        return self._update(sample_size, buffer, lambda batch: self._update_with_batch(batch))


def build(obs_dim, act_dim, latent_dim, hidden=(256, 256), vae_hidden=(512, 512), activation=nn.ReLU, pert_net="mlp", max_action=1.0,
          phi=0.05, **kw):
    """The networks of examples/offline/d4rl_bcq.py:102-148 in its construction order -> BCQ constructor kwargs."""
    k = obs_dim + act_dim
    if pert_net == "mlp":
        net_a = MLP(input_dim=k, output_dim=act_dim, hidden_sizes=list(hidden), activation=activation)
    else:
        net_a = Net(k, list(hidden), activation, act_dim)
    actor = Perturbation(preprocess_net=net_a, max_action=max_action, phi=phi)
    n1, n2 = Net(k, list(hidden), activation), Net(k, list(hidden), activation)
    c1, c2 = SI.ContinuousCritic(n1), SI.ContinuousCritic(n2)
    enc = MLP(input_dim=k, hidden_sizes=list(vae_hidden))
    dec = MLP(input_dim=obs_dim + latent_dim, output_dim=act_dim, hidden_sizes=list(vae_hidden))
    vae = VAE(encoder=enc, decoder=dec, hidden_dim=vae_hidden[-1], latent_dim=latent_dim, max_action=max_action)
    return dict(policy=BCQPolicy(actor_perturbation=actor, critic=c1, vae=vae), critic2=c2, **kw)
