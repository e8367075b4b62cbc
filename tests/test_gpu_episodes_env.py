"""DeviceEpisodes with the rules of the reference's other three environment classes (refills, the scaffold hull, sampled
formulas) against the host loop they replace: `step_canvas` with the same seeds plus the rules environments of
tests/episode_rules_ref.py, step by step, for both agents."""
import numpy as np
import pytest
import torch

from molgym_amd.episodes import DeviceEpisodes, sample_molecules
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import MODEL_DEFAULTS
from tests import episode_rules_ref as X

pytestmark = pytest.mark.gpu
STEPS, E = 24, 6
MAX_SOLO = 2.0
ZS4, ZS5 = [0, 1, 6, 8], [0, 1, 6, 8, 16]
WATER = ((3, (0.0, 0.0, 0.0)), (1, (0.76, 0.59, 0.0)), (1, (-0.76, 0.59, 0.0)))
OCTA = tuple((4, tuple(2.5 * x for x in p)) for p in ((1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)))
FORMULA_SEED = 321
# per mode: zs, canvas size, formulas (FormulaType), their bags, start structure, minimum distance, DeviceEpisodes keywords
MODES = {
    'refill': dict(zs=ZS4, canvas=8, formulas=[((1, 2), (8, 1)), ((6, 1), (1, 4))], bags=[(0, 2, 0, 1), (0, 4, 1, 0)], start=WATER,
                   min_d=1.0, kw=dict(num_refills=2)),
    'hull': dict(zs=ZS5, canvas=10, formulas=[((1, 2), (8, 1)), ((6, 1), (1, 4))], bags=[(0, 2, 0, 1, 0), (0, 4, 1, 0, 0)], start=OCTA,
                 min_d=1.0, kw=dict(scaffold_z=16)),
    'sampled': dict(zs=ZS4, canvas=6, formulas=[((6, 1), (1, 4), (8, 1))], bags=[(0, 4, 1, 1)], start=(), min_d=1.0,
                    kw=dict(size_range=(2, 5), formula_seed=FORMULA_SEED)),
}


def _agent(kind, seed, zs, canvas):
    torch.manual_seed(seed)
    if kind == 'covariant':
        from molgym_amd.agents.covariant import CovariantAC
        return CovariantAC(ObservationSpace(canvas, zs), ActionSpace(zs), bag_scale=5, beta=-10.0, device='cuda:0', **MODEL_DEFAULTS)
    from molgym_amd.agents.internal import SchNetAC
    return SchNetAC(ObservationSpace(canvas, zs), ActionSpace(zs), (0.8, 1.8), 128, device='cuda:0')


def _episodes(mode, ac):
    m = MODES[mode]
    initial = None if not m['start'] else (tuple(m['start']) + ((0, (0.0, 0.0, 0.0)), ) * (m['canvas'] - len(m['start'])), m['bags'][0])
    return DeviceEpisodes(ac, m['formulas'], E, initial=initial, min_atomic_distance=m['min_d'], max_solo_distance=MAX_SOLO, **m['kw'])


def _envs(mode):
    m = MODES[mode]
    kw = dict(num_refills=m['kw'].get('num_refills', 0), scaffold_z=m['kw'].get('scaffold_z'))
    out = []
    for e in range(E):
        if mode == 'sampled':
            lo, hi = m['kw']['size_range']
            kw.update(sampler=dict(counts=m['bags'][0], size_min=lo, size_max=hi, max_tries=64), draw_key=(FORMULA_SEED, e))
        out.append(X.RulesEnvX(m['canvas'], m['zs'], m['bags'], m['min_d'], MAX_SOLO, start=m['start'], **kw))
    return out


def run_equivalence(mode, kind, agent_seed):
    """DeviceEpisodes.step against the host loop, step by step; returns (histogram of the statuses, episodes, what the host
    environments say of each: (env, first formula, refills, bag given))"""
    m = MODES[mode]
    ac = _agent(kind, agent_seed, m['zs'], m['canvas'])
    eps, envs = _episodes(mode, ac), _envs(mode)
    F = len(m['bags'])
    obs = [env._obs() for env in envs]
    cv = ac.make_canvas(obs)
    assert eps.canvas.matches(obs)
    hist, episodes, told = np.zeros(10, dtype=np.int64), [], []
    for t in range(STEPS):
        seed = 1000 * (agent_seed + 1) + t
        with torch.no_grad():
            want = ac.step_canvas(cv, seed=seed)
            got = eps.step(seed=seed)
        status, terminals = [], []
        for e, env in enumerate(envs):
            env.draw_key = (seed, e)  # a formula drawn at this step's reset is keyed by this step's seed
            obs[e], _, done, info = env.step(want['actions'][e])
            status.append(info['status'])
            terminals.append(done)
            if done:
                told.append((e, env.first_formula % F, env.refills, tuple(env.given)))
                obs[e] = env.reset()
        stale = cv.stale_rows(obs, terminals)
        cv.sync(stale, [obs[i] for i in stale])
        assert np.array_equal(got['status'], np.array(status, dtype=np.int32)), t
        assert np.array_equal(got['element'], np.array([a[0] for a in want['actions']], dtype=np.int32)), t
        assert np.array_equal(got['newpos'], np.array([a[1] for a in want['actions']], dtype=np.float64)), t
        assert torch.equal(got['logp'], want['logp'].cpu()) and torch.equal(got['v'], want['v'].cpu()), t
        # the device canvases are the environments' canvases, and the host mirrors are the device arrays
        assert cv.matches(obs) and eps.canvas.matches(obs), t
        assert np.array_equal(eps.canvas.natoms, eps.canvas.natoms_dev.cpu().numpy())
        assert np.array_equal(eps.canvas.bags_host, eps.canvas.bags.cpu().numpy().astype(np.int64))
        assert np.array_equal(eps.canvas.bags_host, [env.bag for env in envs])
        assert np.array_equal(eps.episode_no, eps.episode_no_dev.cpu().numpy()) and np.array_equal(eps.episode_no, [env.episode for env in envs])
        assert np.array_equal(eps.formula_no, eps.formula_no_dev.cpu().numpy()) and np.array_equal(eps.formula_no, [env.formula_no for env in envs])
        assert np.array_equal(eps.refills, eps.refills_dev.cpu().numpy()) and np.array_equal(eps.refills, [env.refills for env in envs])
        hist += np.bincount(got['status'], minlength=10)
        episodes.extend(got['episodes'])
    assert hist[X.ERROR] == 0 and hist[X.INACTIVE] == 0
    assert [(a.env, a.formula, a.refills, a.bag) for a in episodes] == told
    return hist, episodes


def _same(a, b):
    return (a.env, a.formula, a.status, a.refills, a.bag) == (b.env, b.formula, b.status, b.refills, b.bag) and \
        np.array_equal(a.numbers, b.numbers) and np.array_equal(a.positions, b.positions) and np.array_equal(a.logp, b.logp) and \
        np.array_equal(a.v, b.v)


def _same_after_reset(mode, kind, agent_seed):
    m = MODES[mode]
    eps = _episodes(mode, _agent(kind, agent_seed, m['zs'], m['canvas']))
    first = eps.run(num_steps=STEPS, seed=5)
    eps.reset()
    second = eps.run(num_steps=STEPS, seed=5)
    assert len(first) > 0 and len(first) == len(second) and all(_same(a, b) for a, b in zip(first, second))
    return first


# agent seeds whose 24 steps show what the mode is about (asserted below)
SEEDS = {('refill', 'covariant'): 0, ('refill', 'internal'): 1, ('hull', 'covariant'): 0, ('hull', 'internal'): 0,
         ('sampled', 'covariant'): 0, ('sampled', 'internal'): 0}


@pytest.mark.parametrize('kind', ['covariant', 'internal'])
def test_refills_equal_the_host_loop(built_lib, kind):
    hist, episodes = run_equivalence('refill', kind, SEEDS['refill', kind])
    assert hist[X.REFILLED] > 0 and len(episodes) > 0, hist  # (not vacuous)
    for a in episodes:
        assert list(a.numbers[:3]) == [8, 1, 1] and 0 <= a.refills <= 2
        counts = [int(np.sum(a.numbers[3:] == z)) for z in ZS4]
        assert all(c <= b for c, b in zip(counts, a.bag))
    _same_after_reset('refill', kind, SEEDS['refill', kind])


@pytest.mark.parametrize('kind', ['covariant', 'internal'])
def test_hull_equals_the_host_loop(built_lib, kind):
    hist, episodes = run_equivalence('hull', kind, SEEDS['hull', kind])
    assert hist[X.OUTSIDE] > 0 and hist[X.PLACED] > 0, hist
    scaffold = np.array([p for _, p in OCTA])
    episodes = episodes + _same_after_reset('hull', kind, SEEDS['hull', kind])
    placed = 0
    for a in episodes:  # every placed atom of every molecule passes the reference's own test (environment.py:167-171)
        assert np.array_equal(a.positions[:6], scaffold) and list(a.numbers[:6]) == [16] * 6 and 16 not in a.numbers[6:]
        if len(a.numbers) > 6:
            assert np.all(X.inside_scaffold_reference(scaffold, a.positions[6:]))
            placed += len(a.numbers) - 6
    assert placed > 0


@pytest.mark.parametrize('kind', ['covariant', 'internal'])
def test_sampled_formulas_equal_the_host_loop(built_lib, kind):
    hist, episodes = run_equivalence('sampled', kind, SEEDS['sampled', kind])
    assert len({a.bag for a in episodes}) >= 2, hist
    for a in episodes:
        assert 2 <= sum(a.bag) < 5 and a.formula == 0 and a.refills == 0
        assert sum(c * X.BOND_COUNT[z] for c, z in zip(a.bag, ZS4) if c) % 2 == 0
        assert all(int(np.sum(a.numbers == z)) <= b for z, b in zip(ZS4, a.bag))
    _same_after_reset('sampled', kind, SEEDS['sampled', kind])
    m = MODES['sampled']
    mols = sample_molecules(_agent(kind, 1, m['zs'], m['canvas']), m['formulas'], 4, num_envs=3, seed=11, min_atomic_distance=1.0, **m['kw'])
    assert len(mols) == 4 and all(a.status in X.DONE for a in mols)
