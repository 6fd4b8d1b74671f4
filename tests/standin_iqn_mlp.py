"""Minimal stand-ins for the IQN-MLP tests (the reference package is absent on the GPU box): tests/standin_iqn.py's IQN classes over the
`Net` of tests/standin_dqn_mlp.py (real state_dict keys: tests/test_oracle_iqn_mlp.py)."""
from tests.standin_iqn import *  # noqa: F401,F403  (make_hip_iqn_mlp(ref=...) resolves every name in one namespace)
from tests.standin_dqn_mlp import Net as _Net
from tests.standin_iqn import ImplicitQuantileNetwork


class Net(_Net):  # noqa: F811
    def get_output_dim(self):
        return self.model.output_dim


def build(layers, **kw) -> ImplicitQuantileNetwork:
    obs_dim, trunk, feat, n_cos, hidden, n_act = layers
    net = Net(**{**dict(state_shape=obs_dim, action_shape=feat, hidden_sizes=list(trunk)), **kw})
    return ImplicitQuantileNetwork(preprocess_net=net, action_shape=n_act, hidden_sizes=list(hidden), num_cosines=n_cos)
