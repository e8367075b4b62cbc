"""The end of an episode is ONE device function and ONE host mirror (episode.inc: ep_end_episode; episodes.py: _mirror_end).

`mg_episode_cut` against the step's own terminal branch: from one hand-filled state a row that STOPs through the step kernel and
a row that places a legal atom and is then cut must agree, bit for bit, in every array the reset owns.  And after every step of
a `collect`, the host mirrors against the device arrays they mirror, with ends, refills and cuts all counted."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd.rollout import DeviceRollout
from tests import episode_ref as R
from tests import episode_rules_ref as X
from tests import test_gpu_episode_rules as B
from tests import traj_ref as J
from tests.test_gpu_device_rollout import MIN_REWARD, reward_fn
from tests.test_gpu_episodes import CANVAS, FORMULAS, MAX_SOLO, MIN_D, STEPS, WATER, _agent

pytestmark = pytest.mark.gpu
DEV, GUARD = B.DEV, B.GUARD
RESET_OWNS = ('pos64', 'pos32', 'charges', 'bags', 'natoms', 'episode_no')


def _cut_state(N, rules):
    """E = 5 rows on a canvas of N, Z = 4, F = 3.  Rows 0 / 2 take STOP; rows 1 / 3 share their start rows and counters, take a
    legal carbon far from everything (PLACED; row 3 in rules mode REFILLED: its bag holds that one carbon) and are flagged for
    the cut; row 4 places and is not flagged.  Slots beyond a row's atoms hold the candidate's position and a carbon."""
    rng = np.random.default_rng(N)
    E, Z, F = 5, 4, 3
    q = np.array([0.25, -0.5, 0.75])
    n_start = N - 4 if N > 4 else 1
    natoms = np.array([n_start + 2, n_start + 1, n_start + 1, n_start, n_start + 1], dtype=np.int32)
    assert natoms[[1, 3, 4]].max() + 1 < N  # (the placing rows neither fill the canvas nor lack a slot)
    pos64 = np.tile(q, (E, N, 1))
    for e in range(E):
        pos64[e, :natoms[e]] = [(40.0 + 2.0 * i, 8.0 + e, 0.0) for i in range(natoms[e])]
    bags = np.tile(np.array([0, 2, 2, 1], dtype=np.float32), (E, 1))
    if rules:
        bags[3] = (0, 0, 1, 0)
    pair = [0, 0, 2, 2, 4]  # rows of a pair start from the same row
    st = dict(pos64=pos64, pos32=pos64.astype(np.float32), charges=np.full((E, N), 6, dtype=np.int32), bags=bags, natoms=natoms,
              alive=np.ones(E, dtype=np.int32), episode_no=np.array([4, 4, 2, 2, 9], dtype=np.int32),
              start_pos64=rng.uniform(-2.0, 2.0, size=(E, N, 3))[pair], start_charges=rng.choice([1, 6, 8], size=(E, N)).astype(np.int32)[pair],
              start_natoms=np.full(E, n_start, dtype=np.int32), formulas=np.array([(0, 2, 0, 1), (0, 4, 1, 0), (0, 1, 1, 1)], dtype=np.float32))
    if rules:  # row 3's refill moves its cycle position on by one before the cut does: row 2 starts one ahead
        st.update(refills=np.array([1, 1, 1, 0, 1], dtype=np.int32), formula_no=np.array([7, 7, 6, 5, -4], dtype=np.int32))
    acts = np.zeros((E, 7), dtype=np.float32)
    acts[:, 2] = (0, 2, 0, 2, 2)  # zs [0, 1, 6, 8]: STOP or a carbon
    return st, acts, np.tile(q, (E, 1))


@pytest.mark.parametrize('N', [4, 70])
@pytest.mark.parametrize('rules', [False, True])
def test_cut_equals_the_terminal_step(built_lib, rules, N):
    zs, T, t, min_reward = [0, 1, 6, 8], 2, 1, -0.75
    st, acts, newpos = _cut_state(N, rules)
    E, Z, F = 5, len(zs), len(st['formulas'])
    host = dict(st, actions=acts, newpos=newpos, status=np.full(E, -99, dtype=np.int32), element=np.full(E, -99, dtype=np.int32))
    dev = {k: B._guarded(v) for k, v in host.items()}
    ptr = lambda k: C.c_void_p(dev[k].data_ptr() + GUARD * dev[k].element_size())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rows = [ptr(k) for k in ('pos64', 'pos32', 'charges', 'bags', 'natoms', 'alive', 'episode_no', 'start_pos64', 'start_charges',
                             'start_natoms', 'formulas')]

    def read():
        got = {}
        for k, tensor in dev.items():
            flat = tensor.cpu().numpy()
            band = B._poison(flat.dtype)
            assert np.all(flat[:GUARD] == band) and np.all(flat[-GUARD:] == band), f'guard band of {k} overwritten'
            got[k] = torch.from_numpy(flat[GUARD:-GUARD].reshape(host[k].shape).copy())
        return got

    with torch.cuda.device(DEV):
        args = (E, N, Z, F, 7, 0, (C.c_int32 * Z)(*zs), B.MIN_D, B.MAX_SOLO, ptr('actions'), ptr('newpos'), *rows, ptr('status'), ptr('element'))
        if rules:
            r = _lib.EpisodeRules()
            r.num_refills, r.refills, r.formula_no = 1, ptr('refills').value, ptr('formula_no').value
            _lib.check(_lib.lib().mg_episode_step_rules(*args, C.byref(r), stream))
        else:
            _lib.check(_lib.lib().mg_episode_step(*args, stream))
        torch.cuda.synchronize()
        stepped = read()
        status = stepped['status'].numpy()
        assert list(status) == [R.STOP, R.PLACED, R.STOP, X.REFILLED if rules else R.PLACED, R.PLACED]
        assert stepped['natoms'].tolist() == [st['start_natoms'][0], st['natoms'][1] + 1, st['start_natoms'][2], st['natoms'][3] + 1, st['natoms'][4] + 1]
        # the store's slots of step t: the statuses the step wrote, a reward of 0.125
        slots = np.full(E * T, -99, dtype=np.int32)
        slots[t::T] = status
        dev.update(s_status=B._guarded(slots), s_rew=B._guarded(np.full(E * T, 0.125)), flags=B._guarded(np.array([0, 1, 0, 1, 0], dtype=np.int32)))
        host.update(s_status=slots, s_rew=np.full(E * T, 0.125), flags=np.zeros(E, dtype=np.int32))
        counters = (ptr('refills'), ptr('formula_no')) if rules else (None, None)
        _lib.check(_lib.lib().mg_episode_cut(E, N, Z, F, T, t, ptr('flags'), min_reward, *rows, *counters, ptr('s_status'), ptr('s_rew'), stream))
        torch.cuda.synchronize()
    cut = read()
    for k in RESET_OWNS + (('formula_no', 'refills') if rules else ()):
        assert torch.equal(cut[k][1], cut[k][0]) and torch.equal(cut[k][3], cut[k][2]), k  # the cut row equals the stopped row
        assert torch.equal(cut[k][[0, 2, 4]], stepped[k][[0, 2, 4]]), k  # rows that were not flagged are as the step left them
    for e in (1, 3):  # (and what they agree on is the reset, not what the step left)
        assert torch.equal(cut['pos64'][e], torch.from_numpy(st['start_pos64'][e])) and cut['natoms'][e] == st['start_natoms'][e]
        assert not torch.equal(stepped['pos64'][e], cut['pos64'][e]) and not torch.equal(stepped['bags'][e], cut['bags'][e])
    assert cut['episode_no'].tolist() == [5, 5, 3, 3, 9]
    assert torch.equal(cut['bags'][:4], torch.from_numpy(st['formulas'][[8 % 3, 8 % 3, 7 % 3, 7 % 3] if rules else [5 % 3, 5 % 3, 3 % 3, 3 % 3]]))
    if rules:
        assert cut['formula_no'].tolist() == [8, 8, 7, 7, -4] and cut['refills'].tolist() == [0, 0, 0, 0, 1]
    want_status, want_rew = slots.copy(), np.full(E * T, 0.125)
    want_status[[1 * T + t, 3 * T + t]], want_rew[[1 * T + t, 3 * T + t]] = J.LOW_REWARD, min_reward
    assert np.array_equal(cut['s_status'].numpy(), want_status) and np.array_equal(cut['s_rew'].numpy(), want_rew)


# per configuration: DeviceRollout keywords, the start structure, the minimum atomic distance, (agent seed, collect seed).  The
# stand-in reward is the smallest distance to the atoms before minus 1.6: MIN_REWARD = -0.25 cuts what is placed closer than
# 1.35, and -0.5 what is placed closer than 1.1, which leaves episodes that are refilled and go on to fill the canvas
MIRROR_CASES = {
    'default': (dict(), WATER, 1.0, (0, 11)),
    'refill': (dict(num_refills=1), (), 1.0, (1, 11)),
    'cut': (dict(reward_fn=reward_fn), WATER, MIN_D, (0, 11)),
    'refill_cut': (dict(num_refills=1, reward_fn=reward_fn, min_reward=-0.5), (), 1.0, (3, 12)),
}


@pytest.mark.parametrize('case', list(MIRROR_CASES))
def test_mirror_equals_device_after_every_step(built_lib, case):
    """E = 5 on the canvas of 6, 24 steps: before every step's launches (so behind the step, the payment and the cut of the one
    before) and behind the last, every host mirror equals the device array it mirrors.  A start of water leaves three slots,
    so an episode that survives ends FULL; from the empty canvas H2O empties first and is refilled."""
    kw, start, min_d, (agent_seed, seed) = MIRROR_CASES[case]
    kw, E = dict(kw), 5
    min_reward = kw.pop('min_reward', MIN_REWARD)
    ac = _agent('covariant', agent_seed)
    initial = None if not start else (tuple(start) + ((0, (0.0, 0.0, 0.0)), ) * (CANVAS - len(start)), (0, 2, 0, 1))
    roll = DeviceRollout(ac, FORMULAS, E, STEPS, min_reward=min_reward, initial=initial, min_atomic_distance=min_d,
                         max_solo_distance=MAX_SOLO, **kw)
    checks = []

    def compare():
        cv = roll.canvas
        pairs = [('natoms', cv.natoms, cv.natoms_dev), ('bags', cv.bags_host, cv.bags), ('episode_no', roll.episode_no, roll.episode_no_dev)]
        if roll.rules:
            pairs += [('formula_no', roll.formula_no, roll.formula_no_dev), ('refills', roll.refills, roll.refills_dev)]
        for name, mirror, device in pairs:
            assert np.array_equal(np.asarray(mirror, dtype=np.int64), device.cpu().numpy().astype(np.int64)), (name, len(checks))
        checks.append((roll.episode_no.sum(), roll.refills.sum()))

    hooks_of = roll._hooks

    def hooks_and_compare(t, T, v):
        compare()
        return hooks_of(t, T, v)

    roll._hooks = hooks_and_compare
    with torch.no_grad():
        roll.collect(STEPS, seed=seed)
    compare()
    assert len(checks) == STEPS + 1
    hist = np.bincount(roll.statuses().reshape(-1), minlength=11)
    print(case, 'statuses:', {n: int(c) for n, c in zip(('INACTIVE', 'PLACED', 'STOP', 'TOO_CLOSE', 'SOLO', 'FULL', 'BAG_EMPTY', 'ERROR',
                                                        'REFILLED', 'OUTSIDE', 'LOW_REWARD'), hist) if c})
    assert hist[J.ERROR] == 0 and hist[J.INACTIVE] == 0
    assert hist[R.STOP] + hist[R.FULL] > 0 and int(roll.episode_no.sum()) == sum(hist[s] for s in J.ENDS)  # the shared mirror was reached
    if 'num_refills' in kw:
        assert hist[X.REFILLED] > 0
    if 'reward_fn' in kw:
        assert hist[J.LOW_REWARD] > 0
