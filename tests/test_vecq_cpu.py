"""CPU: what the six vector-observation Q engine modules share (tianshou_amd.vecq).  The layout numbers of every family are the ones
the library reported before the shared carve (update_scratch) and the shared Python layout helper existed; every engine's batch-size
refusal names its own family; a refused argument or a refused library call moves no counter."""
from types import SimpleNamespace

import pytest
import torch

from tianshou_amd import _lib
from tianshou_amd import c51_mlp, dqn_mlp, fqf_mlp, iqn_mlp, qrdqn_mlp, rainbow_mlp
from tianshou_amd import vecq as V

BATCHES = (1, 32, 33, 4096)
# module -> [(layout arguments before the batch, count, lds_bytes, workspace_bytes at BATCHES)]: each CPU test's shapes and one
# odd shape (obs 3, trunk (32,), 2 actions), recorded from the library as it was before this file existed
LAYOUTS = {
    dqn_mlp: [
        ((4, (128, 128, 128), None, None, 2), 33922, 58880, (276500, 276500, 412192, 17509384)),
        ((8, (128, 128), (128, 128), (128, 128), 4), 84357, 108928, (679980, 679980, 1017412, 43533844)),
        ((6, (128,), (128, 128), (128, 128), 3), 67460, 92160, (544804, 544804, 814648, 34814992)),
        ((3, (32,), None, None, 2), 194, 13440, (6676, 6676, 7456, 105736)),
    ],
    qrdqn_mlp: [
        ((4, (128, 128, 128, 128), 2, 200), 101776, 118912, (819332, 819332, 1226440, 52522048)),
        ((8, (128, 128, 128, 128), 4, 200), 153888, 119424, (1236228, 1236228, 1851784, 79411840)),
        ((3, (32,), 2, 3), 326, 6272, (7732, 7732, 9040, 173848)),
    ],
    c51_mlp: [
        ((4, (128, 128, 128, 128), 2, 51), 63334, 87040, (511796, 511796, 765136, 32685976)),
        ((8, (128, 128, 128, 128), 4, 51), 77004, 87552, (621156, 621156, 929176, 39739696)),
        ((3, (32,), 2, 3), 326, 6656, (7732, 7732, 9040, 173848)),
    ],
    rainbow_mlp: [
        ((4, (128, 128, 128, 128), (), (), 2, 51, True), 89650, 94592, (722324, 722324, 1080928, 46265032)),
        ((8, (128, 128, 128, 128), (), (), 4, 51, True), 116478, 95104, (936948, 936948, 1402864, 60108280)),
        ((5, (96, 160), (64,), (32,), 3, 7, True), 50200, 52352, (406724, 406724, 607528, 25908832)),
        ((5, (64,), (32,), (), 3, 7, False), 3612, 17664, (34020, 34020, 48472, 1869424)),
        ((4, (64,), (), (), 2, 8, True), 3440, 14848, (32644, 32644, 46408, 1780672)),
        ((3, (32,), (), (), 2, 3, True), 722, 7296, (10900, 10900, 13792, 378184)),
    ],
    iqn_mlp: [
        ((4, (64, 64), 64, 64, (), 2), 12930, 72192, (108564, 108564, 160288, 6677512)),
        ((8, (128, 128), 128, 64, (), 4), 43012, 113664, (349220, 349220, 521272, 22199824)),
        ((3, (32,), 0, 8, (), 2), 482, 35968, (8980, 8980, 10912, 254344)),
    ],
    fqf_mlp: [
        (((4, (64, 64), 64, 64, (64, 64, 64), 2), 32), 25410, 139136, (228744, 228744, 338704, 14194944)),
        (((3, (32,), 0, 8, (), 2), 8), 482, 77952, (14760, 14760, 17744, 395008)),
    ],
}
ENGINES = {dqn_mlp.DQNMlpEngine: "DQN MLP", qrdqn_mlp.QRDQNMlpEngine: "QRDQN MLP", c51_mlp.C51MlpEngine: "C51 MLP",
           rainbow_mlp.RainbowMlpEngine: "Rainbow MLP", iqn_mlp.IQNMlpEngine: "IQN MLP", fqf_mlp.FQFMlpEngine: "FQF MLP"}


@pytest.mark.parametrize("mod", LAYOUTS, ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_layout_numbers_are_the_recorded_ones(mod):
    for args, count, lds, workspace in LAYOUTS[mod]:
        args = args if mod is fqf_mlp else (args,)
        for batch, ws in zip(BATCHES, workspace):
            got = mod.layout(*args, batch)
            assert (got["count"], got["lds_bytes"], got["workspace_bytes"]) == (count, lds, ws), (args, batch)


def test_the_carve_of_the_update_workspace_fits_the_reported_size():
    """update_scratch (ts_mlp_tile.h): slabs | partials | grad_ws | norm_part [1024], each but the first on a 64-float boundary."""
    r64 = lambda n: (n + 63) // 64 * 64  # noqa: E731
    for args, count, _, workspace in LAYOUTS[dqn_mlp] + LAYOUTS[rainbow_mlp]:
        for batch, ws in zip(BATCHES, workspace):
            tiles = (batch + 31) // 32
            assert (tiles * count + r64(tiles) + r64(count) + 1024) * 4 <= ws


@pytest.mark.parametrize("cls", ENGINES, ids=lambda c: c.__name__)
def test_a_batch_outside_the_envelope_is_refused_under_the_engines_own_name(cls):
    assert cls.FAMILY.who == ENGINES[cls]
    stub = SimpleNamespace(obs_dim=3, device="cpu", FAMILY=cls.FAMILY)
    assert cls._obs(stub, torch.zeros(7, 3)).shape == (7, 3)
    with pytest.raises(NotImplementedError, match=f"^{ENGINES[cls]}: a batch of 5000 rows"):
        cls._obs(stub, torch.zeros(5000, 3))
    with pytest.raises(NotImplementedError, match=f"^{ENGINES[cls]}: frame stacking"):
        cls._obs_pair(stub, None, None, None, 1, stack_num=4)


class _Probe(V.VecQEngine):
    """An engine whose library call is `self.call`: update_with_batch as vecq.VecQEngine's docstring lays it out."""
    FAMILY = V.Family("Probe MLP", "nothing")

    def update_with_batch(self, obs, act, weight=None, grad_out=None, apply=True):
        obs = self._obs(obs)
        act, weight = self._batch_args(obs.shape[0], act, weight, grad_out)
        _lib.check(self.call(self._sync_now(), self._adam_arg(apply).value))
        self._stepped(apply)


def test_a_refused_argument_or_library_call_leaves_the_counters_alone():
    eng, seen = _Probe.__new__(_Probe), []
    eng.obs_dim, eng.device, eng.P, eng.cfg = 3, torch.device("cpu"), 5, SimpleNamespace(target_update_freq=2)
    eng.params_old, eng.iter, eng.adam_step = torch.zeros(5), 4, 0
    eng.call = lambda sync, step: seen.append((sync, step)) or _lib.TS_ERR_INVALID_ARG
    obs, act = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    for bad in (dict(act=act[:3]), dict(weight=torch.ones(5)), dict(grad_out=torch.zeros(4)), dict(grad_out=torch.zeros(5, dtype=torch.float64))):
        with pytest.raises(ValueError):
            eng.update_with_batch(obs, **{"act": act, **bad})
    assert not seen
    with pytest.raises(_lib.EngineError):
        eng.update_with_batch(obs, act, torch.ones(4), torch.zeros(5))
    assert seen == [(True, 1)] and (eng.iter, eng.adam_step) == (4, 0)
    eng.call = lambda sync, step: seen.append((sync, step)) or 0
    eng.update_with_batch(obs, act, apply=False)                  # a gradient-only call: the sync is due, Adam's step stays
    eng.update_with_batch(obs, act)
    eng.update_with_batch(obs, act)
    eng.update_with_batch(obs, act, apply=False)
    assert seen[1:] == [(True, 1), (False, 1), (True, 2), (False, 2)] and (eng.iter, eng.adam_step) == (8, 2)
    eng.params_old = None
    assert not eng._sync_now()
