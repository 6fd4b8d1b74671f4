"""CPU: what tianshou_amd.rainbow_mlp accepts and refuses (over the stand-in Net), and its converters."""
import pytest
import torch
from torch import nn

from tests import oracle_rainbow_mlp as OR
from tests import standin_rainbow_mlp as SR
from tianshou_amd import rainbow_mlp as M

SHAPES = {"test_rainbow": (4, (128,) * 4, (), (), 2, 51, True), "lunarlander": (8, (128,) * 4, (), (), 4, 51, True),
          "streams": (5, (96, 160), (64,), (32,), 3, 7, True), "plain": (5, (64,), (32,), (), 3, 7, False)}
SMALL = (4, (64,), (), (), 2, 8, True)


@pytest.mark.parametrize("name", SHAPES)
def test_describe_module_accepts(name):
    layers = SHAPES[name]
    net = SR.build(layers)
    assert M.describe_module(net) == layers
    assert [k for k, p in net.named_parameters() if p.requires_grad] == M.state_dict_keys(layers) == list(OR.init_params(layers, 0))
    assert [k for k in net.state_dict() if "eps_" in k] == M.noise_keys(layers) == list(OR.draw_eps(layers, 0))
    lay = M.layout(layers, 128)
    assert lay["count"] == sum(p.numel() for p in net.parameters() if p.requires_grad) and lay["lds_bytes"] <= 160 * 1024
    assert lay["noise_count"] == sum(net.state_dict()[k].numel() for k in M.noise_keys(layers))


def _mixed():
    net = SR.build(SMALL)
    net.V.model[0] = nn.Linear(64, 8)
    return net


@pytest.mark.parametrize("why,net", [
    ("softmax=True is needed", lambda: SR.build(SMALL, softmax=False)),
    ("dueling_param is needed", lambda: SR.build(SMALL, dueling_param=None)),
    ("no norm_layer", lambda: SR.build(SMALL, norm_layer=nn.LayerNorm)),
    ("activation must be ReLU", lambda: SR.build(SMALL, activation=nn.Tanh)),
    ("found a mix", _mixed),
    ("num_atoms = 1 ", lambda: SR.build(SMALL[:5] + (1, True))),
    ("num_atoms = 257", lambda: SR.build(SMALL[:5] + (257, True))),
    ("width 100", lambda: SR.build((4, (64,), (100,), (), 2, 8, True))),
    ("33 actions", lambda: SR.build((4, (64,), (), (), 33, 8, True))),
    ("2 / 0 hidden layers", lambda: SR.build((4, (64,), (32, 32), (), 2, 8, True))),
    ("at least one trunk hidden layer", lambda: SR.build((4, (), (), (), 2, 8, True))),
    (r"need 334464 bytes of LDS", lambda: SR.build((4, (256,) * 4, (256,), (256,), 2, 256, True))),      # make_net's refused shape + 256 B
])
def test_describe_module_refuses_with_a_reason(why, net):
    with pytest.raises(NotImplementedError, match=why):
        M.describe_module(net())


@pytest.mark.parametrize("name", SHAPES)
def test_flat_and_noise_round_trip(name):
    layers = SHAPES[name]
    x = [p.float() for p in OR.init_params(layers, 1).values()]
    flat = M.flat_from_torch(x, *layers, "cpu")
    assert flat.numel() == M.layout(layers)["count"]
    back = M.flat_to_torch(flat, *layers)
    assert len(back) == len(x) and all(torch.equal(a, b) for a, b in zip(x, back))
    eps = list(OR.draw_eps(layers, 2).values())
    noise = M.noise_from_torch(eps, *layers, "cpu")
    assert noise.numel() == M.layout(layers)["noise_count"] and torch.equal(noise, torch.cat(eps) if eps else noise)
