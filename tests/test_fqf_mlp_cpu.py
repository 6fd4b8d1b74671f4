"""CPU: what tianshou_amd.fqf_mlp accepts and refuses (over the stand-in networks), its converters, the exported symbols and the
layout numbers of test_fqf.py's shape against the carve in ts_fqf_mlp.hip's host comment."""
import pytest
import torch

from tests import oracle_iqn_mlp as OI
from tests import standin_fqf_mlp as SF
from tianshou_amd import _lib
from tianshou_amd import fqf_mlp as M

TEST_FQF = ((4, (64, 64), 64, 64, (64, 64, 64), 2), 32)       # test/discrete/test_fqf.py


def test_layout_of_the_reference_test_shape():
    layers, n = TEST_FQF
    net, frac = SF.build(layers, n)
    assert M.describe_module(net, frac) == (layers, n) and list(net.state_dict()) == M.state_dict_keys(layers) == list(OI.shapes(layers))
    got = M.layout(layers, n, 64)
    assert got["count"] == sum(p.numel() for p in net.parameters()) == 25410
    assert got["fraction_count"] == sum(p.numel() for p in frac.parameters()) == 65 * 32
    assert (got["lds_bytes"], got["F"]) == (34656 * 4 + 512, 64)                       # 139,136 B: the carve of make_fnet


@pytest.mark.parametrize("why,nets", [
    ("4 hidden layers in `last`", lambda: SF.build((4, (64,), 64, 8, (32,) * 4, 2), 8)),
    ("hidden width 48", lambda: SF.build((4, (64,), 64, 8, (32, 32, 48), 2), 8)),
    ("activation must be ReLU", lambda: SF.build((4, (64,), 64, 8, (), 2), 8, activation=torch.nn.Tanh)),
    ("num_fractions = 1 ", lambda: SF.build((4, (64,), 64, 8, (), 2), 1)),
    ("num_fractions = 65", lambda: SF.build((4, (64,), 64, 8, (), 2), 65)),
    ("one Linear", lambda: (SF.build((4, (64,), 64, 8, (), 2), 8)[0], torch.nn.Sequential(torch.nn.Linear(64, 8)))),
    ("reads 32 features", lambda: (SF.build((4, (64,), 64, 8, (), 2), 8)[0], SF.FractionProposalNetwork(8, 32))),
    (r"fraction tables of one 32-row tile need 172160 bytes of LDS", lambda: SF.build((8, (128, 128), 128, 64, (128,), 4), 32)),      # (iqn_mlp takes it)
])
def test_describe_module_refuses_with_a_reason(why, nets):
    net, frac = nets()
    with pytest.raises(NotImplementedError, match=why) as e:
        M.describe_module(net, frac)
    assert "FQF MLP" in str(e.value) and str(e.value).endswith(M.ENVELOPE)      # its own name and envelope, not iqn_mlp's


def test_flat_round_trips_of_both_modules():
    layers, n = TEST_FQF
    torch.manual_seed(0)
    x = [torch.randn(s) for s in OI.shapes(layers).values()]
    flat = M.flat_from_torch(x, *layers, "cpu")
    back = M.flat_to_torch(flat, *layers)
    assert flat.numel() == M.layout(layers, n)["count"] and all(torch.equal(a, b) for a, b in zip(x, back))
    w, b = torch.randn(n, 64), torch.randn(n)
    f = M.fraction_from_torch([w, b], 64, n, "cpu")
    assert torch.equal(f[:64 * n].reshape(64, n), w.t()) and torch.equal(f[64 * n:], b)         # [F + 1, N], row F the bias
    assert all(torch.equal(a, c) for a, c in zip((w, b), M.fraction_to_torch(f, 64, n)))


def test_the_four_entry_points_are_exported_and_refuse_with_unsupported():
    lib = _lib.load()
    for name in ("ts_fqf_mlp_layout", "ts_fqf_mlp_forward", "ts_fqf_mlp_next_dist", "ts_fqf_mlp_update"):
        assert getattr(lib, name).restype is not None and len(getattr(lib, name).argtypes) > 2
    d, out = M._desc((4, (64,), 64, 8, (32, 32, 32), 2), 8), (M.C.c_int64 * 16)()
    assert lib.ts_fqf_mlp_layout(d, 4096, out) == 0 and lib.ts_fqf_mlp_layout(d, 4097, out) == _lib.TS_ERR_UNSUPPORTED
    d[13] = 65
    assert lib.ts_fqf_mlp_layout(d, 1, out) == _lib.TS_ERR_UNSUPPORTED
    assert lib.ts_fqf_mlp_next_dist(None, None, None, d, None, 4, None, None, None, None, None, None, None) == _lib.TS_ERR_UNSUPPORTED
