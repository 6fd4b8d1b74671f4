"""Minimal stand-ins for the C51-MLP tests (the reference package is absent on the GPU box): tests/standin.py's C51 / C51Policy and the
`Net` of tests/standin_dqn_mlp.py with `softmax=True` (real state_dict keys: tests/test_oracle_c51_mlp.py; the softmax of the real
forward is the engine's business, as for tests/standin.py's C51Net)."""
from tests.standin_dqn_mlp import *  # noqa: F401,F403  (make_hip_c51_mlp(ref=...) resolves every name in one namespace)
from tests.standin_dqn_mlp import Net


def build(layers, **kw) -> Net:
    """The Net of a `tianshou_amd.c51_mlp` layers tuple (obs_dim, trunk, n_act, n_atoms)."""
    obs_dim, trunk, n_act, n_atoms = layers
    return Net(**{**dict(state_shape=obs_dim, action_shape=n_act, hidden_sizes=list(trunk), softmax=True, num_atoms=n_atoms), **kw})
