"""SchNetAC training on a rollout that stays on the device (`IntRolloutOnDevice`): its mini-batches against `IntRollout`'s whose
placements were replaced by `mg_int_place`'s (then every member is the same bits), `ppo.train` on
`DeviceRollout.train_data(on_device=True)` against `ppo.train` on that patched host rollout (the same bits in deterministic
mode) and on plain `data()` (the same statistics), the opt-in switches, and the error flag."""
import copy

import numpy as np
import pytest
import torch

import molgym_amd
from molgym_amd import _lib, ppo
from molgym_amd.agents.internal import IntRollout, IntRolloutOnDevice, SchNetAC
from molgym_amd.observations import CarriedRollout
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import make_batch_internal
from tests.helpers import rel_err
from tests.test_gpu_device_rollout import _pair, _train
from tests.test_gpu_internal_canvas import ZS, _agent, _place_dev

pytestmark = pytest.mark.gpu
HP = (0.2, 0.5, 0.01)
_RUNS = {}


@pytest.fixture(autouse=True)
def _restore_switches(built_lib):
    prev = (_lib.is_deterministic(), _lib.is_deterministic_covariant())
    yield
    _lib.set_deterministic(prev[0], covariant=prev[1])


def _patched(ac, data) -> IntRollout:
    """`IntRollout` with the host's float64 placements replaced by mg_int_place's on the same rows"""
    host = IntRollout(ac, data)
    _, _, natoms, pos64 = host.parsed
    plus, minus = _place_dev(pos64, natoms, host.placed[0])
    assert np.abs(plus - host.placed[1]).max() <= 1e-12 and np.abs(minus - host.placed[2]).max() <= 1e-12
    host.placed = (host.placed[0], plus, minus, host.placed[3])
    return host


def _same_batch(a, b):
    for k in ('B', 'N', 'Z', 'W', 'TA', 'MA', 'ME', 'min_distance', 'max_distance'):
        assert getattr(a.cfg, k) == getattr(b.cfg, k), k
    assert list(a.cfg.zs) == list(b.cfg.zs)
    for k in ('mol_off', 'edge_off', 'molZ', 'molpos', 'bags', 'actions', 'logp', 'adv', 'ret'):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), k


def test_from_host_against_the_patched_host_rollout(built_lib):
    ac = _agent(2, canvas=7, width=64)
    data = make_batch_internal(96, 7, ZS, seed=12)
    host, dev = _patched(ac, data), IntRolloutOnDevice.from_host(ac, data)
    perm = np.random.default_rng(1).permutation(96)
    idx_dev = torch.from_numpy(perm).cuda()
    molgym_amd.set_deterministic(True)
    for lo, hi in ((0, 36), (36, 72), (72, 96)):
        a, b = dev.minibatch(perm[lo:hi], idx_dev[lo:hi]), host.minibatch(perm[lo:hi], idx_dev[lo:hi])
        _same_batch(a, b)
        _same_batch(dev.minibatch(perm[lo:hi]), b)  # (and with the index list uploaded by the rollout itself)
        got = []
        for batch in (a, b):
            ac.theta.grad = torch.zeros_like(ac.theta)
            stats = ac.ppo_minibatch(batch, *HP)
            torch.cuda.synchronize()
            got.append((stats.clone(), ac.theta.grad.clone()))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
        assert bool(torch.isfinite(got[0][0]).all()) and float(got[0][1].abs().max()) > 0.0
    dev.check()


def _runs(monkeypatch=None):
    """ppo.train (two epochs, mini-batches of 36 of 144 samples) on the carried form, on the patched host rollout and on plain
    data(), in deterministic and in default mode: each run once"""
    c = _pair('internal', 5, 6)
    if not _RUNS:
        roll = c['roll']
        _RUNS['carried', True] = _train(c['ac'], roll.train_data(on_device=True), True)
        _RUNS['carried', False] = _train(c['ac'], roll.train_data(on_device=True), False)
        _RUNS['data', True] = _train(c['ac'], roll.data(), True)
        _RUNS['data', False] = _train(c['ac'], roll.data(), False)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(SchNetAC, 'prepare_rollout', lambda self, data: _patched(self, data))
            _RUNS['patched', True] = _train(c['ac'], roll.data(), True)
    return c, _RUNS


def test_carried_form_from_a_device_collect(built_lib):
    c, runs = _runs()
    roll, ac = c['roll'], c['ac']
    data = roll.train_data(on_device=True)
    S = len(data['obs'])
    assert isinstance(data['obs'], CarriedRollout) and S == 144 and isinstance(data['obs'].rollout, IntRolloutOnDevice)
    assert ac.prepare_rollout(data) is data['obs'].rollout
    v = roll._views()
    for k, want in (('act', v.actions.view(S, 7)), ('ret', v.ret), ('adv', v.adv), ('logp', v.logp)):
        assert data[k].data_ptr() == want.data_ptr() and torch.equal(data[k], want), k  # views of the store
    assert isinstance(roll.train_data()['obs'], list) and isinstance(roll.train_data(on_device=False)['obs'], list)
    with pytest.raises(ValueError, match='on_device'):
        roll.train_data(on_device=1)
    # deterministic mode: the bits of ppo.train on the host rollout with mg_int_place's placements
    a, b = runs['carried', True], runs['patched', True]
    assert a[0]['num_opt_steps'] == b[0]['num_opt_steps'] == 2 and set(a[0]) == set(b[0])
    for k in a[0]:
        if k != 'time':
            assert a[0][k] == b[0][k], (k, a[0][k], b[0][k])
    assert torch.equal(a[1], b[1]) and not torch.equal(a[1], ac.theta.detach())  # theta moved
    assert a[2] is not None and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    # against plain data() (the host's float64 placements: roundings to float32 may differ by one spacing), in both modes
    for det in (True, False):
        a, b = runs['carried', det], runs['data', det]
        assert a[0]['num_opt_steps'] == b[0]['num_opt_steps'] == 2
        for k in ppo.KEYS:
            print(det, k, a[0][k], b[0][k])
            assert rel_err(torch.tensor(a[0][k]), torch.tensor(b[0][k])) < 1e-5, (det, k, a[0][k], b[0][k])


def test_carried_form_trains_on_three_streams(built_lib, monkeypatch):
    """default mode: the gathers run on the mini-batches' own streams"""
    monkeypatch.delenv('MOLGYM_TRAIN_STREAMS', raising=False)
    c, runs = _runs()
    runner = ppo._DeviceRunner(c['ac'], c['roll'].train_data(on_device=True), 36, HP)
    assert len(runner.streams) == 3 and isinstance(runner.rollout, IntRolloutOnDevice)
    a, b = runs['carried', False], runs['carried', True]
    assert a[0]['num_opt_steps'] == 2 and not torch.equal(a[1], c['ac'].theta.detach())
    for k in ppo.KEYS:
        assert np.isfinite(a[0][k]) and rel_err(torch.tensor(a[0][k]), torch.tensor(b[0][k])) < 1e-5, (k, a[0][k], b[0][k])


def test_gather_on_device_routes_host_data(built_lib, monkeypatch):
    c = _pair('internal', 5, 6)
    data = c['roll'].data()
    ac = copy.deepcopy(c['ac'])
    assert ac.gather_on_device is False and type(ac.prepare_rollout(data)) is IntRollout
    ac.gather_on_device = True
    assert type(ppo._DeviceRunner(ac, data, 36, HP).rollout) is IntRolloutOnDevice
    # parked from the host form: the arrays of the store, so the same mini-batches as the carried form's
    mine, carried = ac.prepare_rollout(data), c['roll'].train_data(on_device=True)['obs'].rollout
    idx = np.random.default_rng(2).permutation(144)[:36]
    _same_batch(mine.minibatch(idx), carried.minibatch(idx))
    mine.check()
    carried.check()
    monkeypatch.setenv('MG_INT_DEVICE_GATHER', '1')
    assert SchNetAC(ObservationSpace(7, ZS), ActionSpace(ZS), (0.8, 1.8), 64, device='cuda:0').gather_on_device is True
    monkeypatch.delenv('MG_INT_DEVICE_GATHER')
    assert SchNetAC(ObservationSpace(7, ZS), ActionSpace(ZS), (0.8, 1.8), 64, device='cuda:0').gather_on_device is False


def test_from_host_refuses_what_the_host_placement_refuses(built_lib):
    ac = _agent(2, canvas=7, width=64)
    data = make_batch_internal(12, 7, ZS, seed=3)
    natoms = ac._parse(data['obs'])[2]
    row = int(np.nonzero((natoms > 0) & (natoms < 7))[0][0])
    bad = dict(data, act=data['act'].copy())
    bad['act'][row, 1] = natoms[row]
    with pytest.raises(RuntimeError, match='Focus greater than number of atoms'):
        IntRolloutOnDevice.from_host(ac, bad)
    for col, value in ((1, 7), (1, -1), (2, len(ZS)), (2, -1)):
        bad = dict(data, act=data['act'].copy())
        bad['act'][row, col] = value
        with pytest.raises(RuntimeError, match='index out of range'):
            IntRolloutOnDevice.from_host(ac, bad)
        with pytest.raises(RuntimeError, match='index out of range'):
            IntRollout(ac, bad)


def test_error_flag_of_a_tampered_mirror(built_lib):
    ac = _agent(2, canvas=7, width=64)
    data = make_batch_internal(48, 7, ZS, seed=5)
    ro = IntRolloutOnDevice.from_host(ac, data)
    idx = np.arange(36)
    ro.minibatch(idx)
    ro.check()  # nothing to report
    row = int(np.nonzero(ro.natoms[:36] < 7)[0][0])
    ro.natoms[row] += 1  # the host mirror no longer is what the device holds
    batch = ro.minibatch(idx)
    with pytest.raises(RuntimeError, match='host mirror'):
        ro.check()
    # the flagged batch lies inside the sizes the host gave
    mol_off, edge_off = batch.mol_off.cpu().numpy(), batch.edge_off.cpu().numpy()
    assert mol_off[0] == 0 and mol_off[-1] == batch.cfg.MA and np.all(np.diff(mol_off) >= 0)
    assert edge_off[0] == 0 and edge_off[-1] <= batch.cfg.ME and np.all(np.diff(edge_off) >= 0)
    assert not bool(batch.molZ.any()) and not bool(batch.molpos.any())
