"""CPU: what tianshou_amd.c51_mlp accepts and refuses (over the stand-in Net), and its converters."""
import pytest
import torch
from torch import nn

from tests import oracle_qrdqn_mlp as OQ
from tests import standin_c51_mlp as SC
from tianshou_amd import c51_mlp as M

SHAPES = {"test_c51": (4, (128,) * 4, 2, 51), "lunarlander": (8, (128,) * 4, 4, 51)}


@pytest.mark.parametrize("name", SHAPES)
def test_describe_module_accepts_the_two_shapes(name):
    layers = SHAPES[name]
    net = SC.build(layers)
    assert M.describe_module(net) == layers
    assert list(net.state_dict()) == M.state_dict_keys(layers)
    lay = M.layout(layers, 128)
    assert lay["count"] == sum(p.numel() for p in net.parameters()) and lay["lds_bytes"] <= 160 * 1024


@pytest.mark.parametrize("why,net", [
    ("softmax=True is needed", lambda: SC.build((4, (64,), 2, 8), softmax=False)),
    ("dueling_param with atoms", lambda: SC.build((4, (64,), 2, 8), dueling_param=({"hidden_sizes": [32]}, {"hidden_sizes": [32]}))),
    ("no norm_layer", lambda: SC.build((4, (64,), 2, 8), norm_layer=nn.LayerNorm)),
    ("activation must be ReLU", lambda: SC.build((4, (64,), 2, 8), activation=nn.Tanh)),
    ("num_atoms = 1 ", lambda: SC.build((4, (64,), 2, 1))),
    ("num_atoms = 257", lambda: SC.build((4, (64,), 2, 257))),
    ("width 100", lambda: SC.build((4, (100,), 2, 8))),
    ("33 actions", lambda: SC.build((4, (64,), 33, 8))),
    ("at least one hidden layer", lambda: SC.build((4, (), 2, 8))),
    (r"need 231680 bytes of LDS", lambda: SC.build((4, (256,) * 4, 2, 256))),       # 32 (5 + 7 x 257) floats + 128 scalars + 256 B
])
def test_describe_module_refuses_with_a_reason(why, net):
    with pytest.raises(NotImplementedError, match=why):
        M.describe_module(net())


@pytest.mark.parametrize("layers", [SHAPES["test_c51"], (5, (96, 160), 3, 7), (17, (32,), 32, 3)])
def test_flat_round_trip(layers):
    torch.manual_seed(0)
    x = [torch.randn(s) for s in OQ.OM.shapes(OQ.plain(layers)).values()]
    flat = M.flat_from_torch(x, *layers, "cpu")
    assert flat.numel() == M.layout(layers)["count"]
    back = M.flat_to_torch(flat, *layers)
    assert len(back) == len(x) and all(torch.equal(a, b) for a, b in zip(x, back))
