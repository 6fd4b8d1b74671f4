"""CPU: what tianshou_amd.qrdqn_mlp accepts and refuses (over the stand-in Net), and its converters."""
import pytest
import torch

from tests import oracle_qrdqn_mlp as OQ
from tests import standin_qrdqn_mlp as SQ
from tianshou_amd import qrdqn_mlp as M

SHAPES = {"test_qrdqn": (4, (128,) * 4, 2, 200), "lunarlander": (8, (128,) * 4, 4, 200)}


@pytest.mark.parametrize("name", SHAPES)
def test_describe_module_accepts_the_two_shapes(name):
    layers = SHAPES[name]
    net = SQ.build(layers)
    assert M.describe_module(net) == layers
    assert list(net.state_dict()) == M.state_dict_keys(layers)
    lay = M.layout(layers, 128)
    assert lay["count"] == sum(p.numel() for p in net.parameters()) and lay["lds_bytes"] <= 160 * 1024


@pytest.mark.parametrize("why,net", [
    ("dueling_param with quantiles", lambda: SQ.build((4, (64,), 2, 8), dueling_param=({"hidden_sizes": [32]}, {"hidden_sizes": [32]}))),
    ("softmax=True is not supported", lambda: SQ.build((4, (64,), 2, 8), softmax=True)),
    ("num_atoms = 1 ", lambda: SQ.build((4, (64,), 2, 1))),
    ("num_atoms = 257", lambda: SQ.build((4, (64,), 2, 257))),
    ("width 100", lambda: SQ.build((4, (100,), 2, 8))),
    ("33 actions", lambda: SQ.build((4, (64,), 33, 8))),
    (r"need 19\d\d\d\d bytes of LDS", lambda: SQ.build((4, (256,) * 4, 2, 256))),
])
def test_describe_module_refuses_with_a_reason(why, net):
    with pytest.raises(NotImplementedError, match=why):
        M.describe_module(net())


@pytest.mark.parametrize("layers", [SHAPES["test_qrdqn"], (5, (96, 160), 3, 7), (17, (32,), 32, 3)])
def test_flat_round_trip(layers):
    torch.manual_seed(0)
    x = [torch.randn(s) for s in OQ.OM.shapes(OQ.plain(layers)).values()]
    flat = M.flat_from_torch(x, *layers, "cpu")
    assert flat.numel() == M.layout(layers)["count"]
    back = M.flat_to_torch(flat, *layers)
    assert len(back) == len(x) and all(torch.equal(a, b) for a, b in zip(x, back))
