"""Minimal stand-ins for the Rainbow-MLP tests (no reference package on the GPU box): tests/standin.py's RainbowDQN / C51Policy / NoisyLinear and the dueling
`Net` of tests/standin_dqn_mlp.py, its stream layers replaced by NoisyLinear as `linear_layer` does (real parameter names: tests/test_oracle_rainbow_mlp.py)."""
from torch import nn

from tests.standin_dqn_mlp import *  # noqa: F401,F403  (make_hip_rainbow_mlp(ref=...) resolves every name in one namespace)
from tests.standin_dqn_mlp import Net, NoisyLinear


def build(layers, noisy_std=0.5, **kw) -> Net:
    """The Net of a `tianshou_amd.rainbow_mlp` layers tuple (obs_dim, trunk, q_hidden, v_hidden, n_act, n_atoms, noisy)."""
    obs_dim, trunk, q, v, n_act, n_atoms, noisy = layers
    net = Net(**{**dict(state_shape=obs_dim, action_shape=n_act, hidden_sizes=list(trunk), softmax=True, num_atoms=n_atoms,
                        dueling_param=({"hidden_sizes": list(q)}, {"hidden_sizes": list(v)})), **kw})
    for mlp in (net.Q, net.V) if noisy and net.use_dueling else ():
        for i, m in enumerate(mlp.model):
            if isinstance(m, nn.Linear):
                mlp.model[i] = NoisyLinear(m.in_features, m.out_features, noisy_std)
    return net
