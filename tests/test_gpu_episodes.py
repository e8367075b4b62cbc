"""DeviceEpisodes: whole episodes on the device (sampling launch + mg_episode_step) against the host loop they replace --
`step_canvas` with the same seeds, the rules environment of tests/episode_ref.py, `stale_rows` / `sync` -- for both agents."""
import numpy as np
import pytest
import torch

from molgym_amd.episodes import DeviceEpisodes, sample_molecules
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import MODEL_DEFAULTS
from tests import episode_ref as R

pytestmark = pytest.mark.gpu
ZS, CANVAS, STEPS = [0, 1, 6, 8], 6, 24
FORMULAS = [((1, 2), (8, 1)), ((6, 1), (1, 4))]  # H2O, CH4 (FormulaType)
BAGS = [(0, 2, 0, 1), (0, 4, 1, 0)]
# mean distances of the policies lie in 0.8 .. 1.8: a minimum distance of 1.2 rejects a good share of the draws
MIN_D, MAX_SOLO = 1.2, 2.0
WATER = ((3, (0.0, 0.0, 0.0)), (1, (0.76, 0.59, 0.0)), (1, (-0.76, 0.59, 0.0)))


def _agent(kind, seed):
    torch.manual_seed(seed)
    if kind == 'covariant':
        from molgym_amd.agents.covariant import CovariantAC
        return CovariantAC(ObservationSpace(CANVAS, ZS), ActionSpace(ZS), bag_scale=5, beta=-10.0, device='cuda:0', **MODEL_DEFAULTS)
    from molgym_amd.agents.internal import SchNetAC
    return SchNetAC(ObservationSpace(CANVAS, ZS), ActionSpace(ZS), (0.8, 1.8), 128, device='cuda:0')


def run_equivalence(kind, training, agent_seed, E, min_d=MIN_D, start=()):
    """DeviceEpisodes.step against the host loop, step by step; returns the histogram of the statuses met"""
    ac = _agent(kind, agent_seed)
    ac.training = training
    initial = None if not start else (tuple(start) + ((0, (0.0, 0.0, 0.0)), ) * (CANVAS - len(start)), BAGS[0])
    eps = DeviceEpisodes(ac, FORMULAS, E, initial=initial, min_atomic_distance=min_d, max_solo_distance=MAX_SOLO)
    envs = [R.RulesEnv(CANVAS, ZS, BAGS, min_d, MAX_SOLO, start=start) for _ in range(E)]
    obs = [env._obs() for env in envs]
    cv = ac.make_canvas(obs)
    assert eps.canvas.matches(obs)
    hist = np.zeros(8, dtype=np.int64)
    for t in range(STEPS):
        seed = 1000 * (agent_seed + 1) + t
        with torch.no_grad():
            want = ac.step_canvas(cv, seed=seed)
            got = eps.step(seed=seed)
        status, terminals = [], []
        for e, env in enumerate(envs):
            obs[e], _, done, info = env.step(want['actions'][e])
            status.append(info['status'])
            terminals.append(done)
            if done:
                obs[e] = env.reset()
        stale = cv.stale_rows(obs, terminals)
        cv.sync(stale, [obs[i] for i in stale])
        assert np.array_equal(got['status'], np.array(status, dtype=np.int32)), t
        assert np.array_equal(got['element'], np.array([a[0] for a in want['actions']], dtype=np.int32)), t
        assert np.array_equal(got['newpos'], np.array([a[1] for a in want['actions']], dtype=np.float64)), t
        assert torch.equal(got['logp'], want['logp'].cpu()) and torch.equal(got['v'], want['v'].cpu()), t
        # the device canvases are the environments' canvases, and the host mirrors are the device counts
        assert cv.matches(obs) and eps.canvas.matches(obs), t
        assert np.array_equal(eps.canvas.natoms, eps.canvas.natoms_dev.cpu().numpy())
        assert np.array_equal(eps.canvas.bags_host, eps.canvas.bags.cpu().numpy().astype(np.int64))
        assert np.array_equal(eps.episode_no, eps.episode_no_dev.cpu().numpy()) and np.array_equal(eps.episode_no, [env.episode for env in envs])
        hist += np.bincount(got['status'], minlength=8)
    return hist


def _covers(hist):
    return hist[R.PLACED] > 0 and hist[R.BAG_EMPTY] > 0 and hist[R.TOO_CLOSE] + hist[R.SOLO] > 0


# (kind, training, agent seed, environments): seeds whose 24 steps meet a placement, a finished molecule and a rejection
# (an evaluation-mode policy is deterministic, so most initial weights give one outcome over and over: these two seeds do not)
CASES = [('covariant', True, 0, 6), ('internal', True, 0, 6), ('covariant', True, 1, 70), ('covariant', False, 1, 6),
         ('internal', False, 5, 6)]


@pytest.mark.parametrize('kind,training,agent_seed,E', CASES)
def test_device_episodes_equal_the_host_loop(built_lib, kind, training, agent_seed, E):
    hist = run_equivalence(kind, training, agent_seed, E)
    assert _covers(hist), hist  # (not vacuous)
    assert hist[R.ERROR] == 0 and hist[R.INACTIVE] == 0


def _same(a, b):
    return (a.env, a.formula, a.status) == (b.env, b.formula, b.status) and np.array_equal(a.numbers, b.numbers) and \
        np.array_equal(a.positions, b.positions) and np.array_equal(a.logp, b.logp) and np.array_equal(a.v, b.v)


@pytest.mark.parametrize('kind', ['covariant', 'internal'])
def test_same_seed_same_episodes(built_lib, kind):
    ac = _agent(kind, 3)
    eps = DeviceEpisodes(ac, FORMULAS, 6, min_atomic_distance=MIN_D)
    first = eps.run(num_steps=STEPS, seed=5)
    eps.reset()
    second = eps.run(num_steps=STEPS, seed=5)
    third = DeviceEpisodes(ac, FORMULAS, 6, min_atomic_distance=MIN_D).run(num_steps=STEPS, seed=5)
    other = DeviceEpisodes(ac, FORMULAS, 6, min_atomic_distance=MIN_D).run(num_steps=STEPS, seed=6)
    assert len(first) > 0 and len(first) == len(second) == len(third)
    assert all(_same(a, b) for a, b in zip(first, second)) and all(_same(a, b) for a, b in zip(first, third))
    assert len(other) != len(first) or not all(_same(a, b) for a, b in zip(first, other))


@pytest.mark.parametrize('kind', ['covariant', 'internal'])
def test_run_num_episodes_returns_the_first_k_of_the_record(built_lib, kind):
    ac = _agent(kind, 4)
    k, E = 5, 6
    # the step record, taken with the seeds run() derives from its seed
    eps = DeviceEpisodes(ac, FORMULAS, E, min_atomic_distance=MIN_D)
    gen = torch.Generator().manual_seed(7)
    records = [eps.step(int(torch.randint(0, 2**62, (1, ), generator=gen).item())) for _ in range(STEPS)]
    want = R.collect_episodes(records, ZS, len(FORMULAS), [[]] * E, [np.zeros((0, 3))] * E)
    assert len(want) > k
    full = DeviceEpisodes(ac, FORMULAS, E, min_atomic_distance=MIN_D).run(num_steps=STEPS, seed=7)
    got = DeviceEpisodes(ac, FORMULAS, E, min_atomic_distance=MIN_D).run(num_episodes=k, seed=7)
    assert len(got) == k and len(full) == len(want)
    for a, w in zip(got + full, want[:k] + want):
        assert (a.env, a.formula, a.status) == (w['env'], w['formula'], w['status'])
        assert np.array_equal(a.numbers, w['numbers']) and np.array_equal(a.positions, w['positions'])
        assert np.array_equal(a.logp, w['logp']) and np.array_equal(a.v, w['v'])
        assert a.positions.dtype == np.float64 and a.positions.shape == (len(a.numbers), 3)
        # every molecule obeys both distance rules and its formula
        assert R.molecule_obeys_rules(ZS, CANVAS, a.numbers, a.positions, BAGS[a.formula], 0, MIN_D, MAX_SOLO)
        counts = [int(np.sum(a.numbers == z)) for z in ZS]
        assert all(c <= b for c, b in zip(counts, BAGS[a.formula]))
        if a.status == R.BAG_EMPTY:
            assert counts == list(BAGS[a.formula])
    mols = sample_molecules(ac, FORMULAS, 4, num_envs=3, seed=11, min_atomic_distance=MIN_D)
    assert len(mols) == 4 and all(m.status in R.DONE for m in mols)


def test_start_structure_is_kept_through_resets(built_lib):
    """every episode starts from water; the rules see its atoms, the reset brings it back"""
    hist = run_equivalence('covariant', True, 2, 6, min_d=1.0, start=WATER)
    assert sum(hist[s] for s in R.DONE) > 0 and hist[R.PLACED] > 0, hist
    ac = _agent('internal', 2)
    initial = (WATER + ((0, (0.0, 0.0, 0.0)), ) * (CANVAS - 3), BAGS[1])
    eps = DeviceEpisodes(ac, FORMULAS, 6, initial=initial, min_atomic_distance=1.0)
    done = eps.run(num_steps=STEPS, seed=1)
    water = np.array([p for _, p in WATER])
    assert len(done) > 0
    for m in done:
        assert list(m.numbers[:3]) == [8, 1, 1] and np.array_equal(m.positions[:3], water)
        assert R.molecule_obeys_rules(ZS, CANVAS, m.numbers, m.positions, BAGS[m.formula], 3, 1.0, MAX_SOLO)
    cv = eps.canvas
    assert np.array_equal(cv.pos64[:, :3].cpu().numpy(), np.tile(water, (6, 1, 1))) and np.all(cv.natoms >= 3)
    assert np.array_equal(cv.charges[:, :3].cpu().numpy(), np.tile([8, 1, 1], (6, 1)))


def test_out_of_scope_and_bad_inputs_raise(built_lib):
    ac = _agent('internal', 0)
    with pytest.raises(ValueError):
        DeviceEpisodes(ac, [((2, 2), )], 4)  # He is not among zs
    with pytest.raises(ValueError):
        DeviceEpisodes(ac, [], 4)
    full = (tuple((1, (float(i), 0.0, 0.0)) for i in range(CANVAS)), BAGS[0])
    with pytest.raises(ValueError):
        DeviceEpisodes(ac, FORMULAS, 2, initial=full)
    with pytest.raises(ValueError):
        DeviceEpisodes(ac, FORMULAS, 2).run()
