"""CPU: what tianshou_amd.dqn_mlp accepts and refuses (over the stand-in Net), and its converters."""
import pytest
import torch
from torch import nn

from tests import oracle_dqn_mlp as OM
from tests import standin_dqn_mlp as SM
from tianshou_amd import dqn_mlp as M

EXAMPLES = {"discrete_dqn": (4, (128, 128, 128), None, None, 2), "lunarlander_dqn": (8, (128, 128), (128, 128), (128, 128), 4),
            "acrobot_dualdqn": (6, (128,), (128, 128), (128, 128), 3)}


@pytest.mark.parametrize("name", EXAMPLES)
def test_describe_module_accepts_the_example_networks(name):
    layers = EXAMPLES[name]
    net = SM.build(layers)
    assert M.describe_module(net) == layers
    assert list(net.state_dict()) == M.state_dict_keys(layers) == list(OM.shapes(layers))
    lay = M.layout(layers, 128)
    assert lay["count"] == sum(p.numel() for p in net.parameters()) and lay["lds_bytes"] <= 160 * 1024


@pytest.mark.parametrize("why,net", [
    ("ReLU", lambda: SM.build(EXAMPLES["lunarlander_dqn"], activation=nn.Tanh)),
    ("multiple of 32", lambda: SM.build((4, (100,), None, None, 2))),
    ("33 actions", lambda: SM.build((4, (64,), (), (), 33))),
    ("num_atoms", lambda: SM.build((4, (64,), None, None, 2), num_atoms=2)),
    ("softmax", lambda: SM.build((4, (64,), None, None, 2), softmax=True)),
    ("5 trunk hidden layers", lambda: SM.build((4, (32,) * 5, None, None, 2))),
    ("bytes of LDS", lambda: SM.build((4, (256,) * 4, (256, 256), (256, 256), 2))),
])
def test_describe_module_refuses_with_a_reason(why, net):
    with pytest.raises(NotImplementedError, match=why):
        M.describe_module(net())


@pytest.mark.parametrize("layers", [EXAMPLES["acrobot_dualdqn"], (5, (96, 160), (32, 96), (160,), 5), (17, (64, 32), None, None, 32)])
def test_flat_round_trip(layers):
    torch.manual_seed(0)
    x = [torch.randn(s) for s in OM.shapes(layers).values()]
    flat = M.flat_from_torch(x, *layers, "cpu")
    assert flat.numel() == M.layout(layers)["count"]
    back = M.flat_to_torch(flat, *layers)
    assert len(back) == len(x) and all(torch.equal(a, b) for a, b in zip(x, back))
