"""The host side of SchNetAC's device gather (`IntRolloutOnDevice`, `DeviceRollout.train_data(on_device=...)`): the totals of a
mini-batch against a brute-force count, their 2^31 refusal, the refusals of the new keyword, and `prepare_rollout` handing back
what a `CarriedRollout` carries.  No GPU."""
import inspect
import types

import numpy as np
import pytest

from molgym_amd import rollout
from molgym_amd.observations import CarriedRollout


def _brute_force(natoms):
    """count the atoms and the ordered pairs of the 3B molecules one by one"""
    TA = MA = ME = 0
    for n in natoms:
        TA += sum(1 for _ in range(n))
        for size in (n, n + 1, n + 1):  # the canvas, the canvas plus the new atom at +dihedral, at -dihedral
            MA += size
            ME += sum(1 for i in range(size) for j in range(size) if i != j)
    return TA, MA, ME


@pytest.mark.parametrize('N,B,seed', [(7, 36, 0), (9, 1, 1), (20, 23, 2), (40, 5, 3)])
def test_totals_against_a_brute_force_count(N, B, seed):
    from molgym_amd.agents.internal import gather_totals
    rng = np.random.default_rng(seed)
    natoms = rng.integers(0, N + 1, size=B)
    natoms[0] = N
    if B > 1:
        natoms[1] = 0
    assert gather_totals(natoms) == _brute_force([int(n) for n in natoms])
    assert gather_totals(natoms.astype(np.int32)) == gather_totals(natoms)  # (summed in int64 whatever comes in)
    assert gather_totals(np.zeros(B, dtype=np.int64)) == (0, 2 * B, 0)


def test_totals_refuse_two_to_the_31_pairs():
    from molgym_amd.agents.internal import gather_totals
    per = 3 * 255 * 255 + 255  # pairs of one full canvas of 255 atoms
    k = -(-2**31 // per)  # the fewest such samples that reach 2^31
    TA, MA, ME = gather_totals(np.full(k - 1, 255, dtype=np.int32))
    assert ME == (k - 1) * per < 2**31 and MA == 3 * TA + 2 * (k - 1)
    with pytest.raises(ValueError, match='2\\^31'):
        gather_totals(np.full(k, 255, dtype=np.int32))  # (an int32 sum would have wrapped to a negative count)


def test_on_device_keyword_values():
    assert rollout.check_on_device(None) is None and rollout.check_on_device(True) is True and rollout.check_on_device(False) is False
    assert rollout.check_on_device(np.bool_(True)) is True
    for bad in (1, 0, 'yes', 'True', 1.0, [True], 'cuda'):
        with pytest.raises(ValueError, match='on_device'):
            rollout.check_on_device(bad)
    par = inspect.signature(rollout.DeviceRollout.train_data).parameters
    assert par['on_device'].default is None


def test_prepare_rollout_returns_what_is_carried():
    from molgym_amd.agents.internal import SchNetAC
    assert SchNetAC.gather_on_device is False
    carried = object()
    for flag in (False, True):
        me = types.SimpleNamespace(gather_on_device=flag)
        assert SchNetAC.prepare_rollout(me, dict(obs=CarriedRollout(3, carried))) is carried
