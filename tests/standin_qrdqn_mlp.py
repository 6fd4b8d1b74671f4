"""Minimal stand-ins for the QRDQN-MLP tests (the reference package is absent on the GPU box): tests/standin.py's QRDQN and the
`Net` of tests/standin_dqn_mlp.py, which takes `num_atoms` (real state_dict keys: tests/test_oracle_qrdqn_mlp.py)."""
from tests.standin_dqn_mlp import *  # noqa: F401,F403  (make_hip_qrdqn_mlp(ref=...) resolves every name in one namespace)
from tests.standin_dqn_mlp import Net


def build(layers, **kw) -> Net:
    """The Net of a `tianshou_amd.qrdqn_mlp` layers tuple (obs_dim, trunk, n_act, n_atoms)."""
    obs_dim, trunk, n_act, n_atoms = layers
    return Net(**{**dict(state_shape=obs_dim, action_shape=n_act, hidden_sizes=list(trunk), num_atoms=n_atoms), **kw})
