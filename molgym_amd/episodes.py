"""Device-resident episodes: sample whole molecules from a policy without host environments.

A trained policy is a generative model, and sampling from it needs no reward: energies are computed afterwards on the
finished structures.  `batch_rollout` over Python environments pays, per environment and step, an `ase.Atoms`, an
observation tuple of `canvas_size` items, a re-upload of every canvas that ended and a reward call whose result is thrown
away -- all around a policy step of a fraction of a millisecond.  Here the canvases stay in HBM (`agents/canvas.py`) and
the environment's rules run there too: one sampling launch (`_sample_canvas`, the launch `step_canvas` issues) and one
`mg_episode_step` (include/molgym_hip.h) per step apply the two distance rules, the bag decrement, the terminal test and
the reset of finished environments of the reference's `MolecularEnvironment` (environment.py:49-118,134-140).

`mg_episode_step_rules`, a second entry point, adds the rules of the reference's other three environment classes.  The two
kernels are the two instantiations of ONE device body, and every end of an episode -- either step's terminal branch and
`mg_episode_cut` -- is one device function, mirrored on the host by `DeviceEpisodes._mirror_end`.  `DeviceEpisodes` calls
the rules entry point only when one of their keywords is given:
  * `num_refills` -- RefillableMolecularEnvironment (environment.py:178-207, scripts/run_solvation.py): an empty bag is refilled
    from the same formula cycle the resets draw from, `num_refills` times per episode;
  * `scaffold_z` -- ConstrainedMolecularEnvironment (:143-175): a new atom must lie inside the convex hull of the start
    structure's atoms of that element.  The hull is computed ONCE, on the host; in the reference a placed atom of the scaffold
    element would join it (:156-157), so a fixed hull is exact only without such atoms and formulas that hold `scaffold_z` are
    refused;
  * `size_range` -- StochasticEnvironment (:210-249, scripts/run_stochastic.py): every reset draws a new formula on the device,
    from the keyed generator of the sampling kernels (the reference draws from numpy's global generator; the distribution is the
    same, the stream is not).  The reference repeats an invalid draw for ever; the device tries `max_formula_tries` times and the
    constructor refuses configurations whose tries are valid with probability below 1/4.

`min_reward` termination (environment.py:58-70) is covered by `DeviceRollout` (molgym_amd/rollout.py), which records the
trajectories of these environments on the device for `ppo.train`: the rule rewards are written there, the caller's reward
function runs on the host (or, for a `rewards.PairReward`, `mg_traj_pair_reward` on the device), and a reward below `min_reward`
cuts the episode (`mg_episode_cut`, status LOW_REWARD).  The one exception is `size_range` together with a reward: a cut would
need a formula draw outside a step.

Data parallelism: `shard=(rank, world)` makes an instance this rank's contiguous share of `num_envs` GLOBAL environments; its
rows draw from the random streams of their global numbers, so the shares of all ranks together are the environments one process
would step (`DeviceRollout.train_data` exchanges the recorded stores).

Not covered, by design: a hull that grows with placed scaffold atoms."""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

DONE_STATUSES = (_lib.EP_STOP, _lib.EP_TOO_CLOSE, _lib.EP_SOLO, _lib.EP_FULL, _lib.EP_BAG_EMPTY, _lib.EP_OUTSIDE)
ATOM_STATUSES = (_lib.EP_PLACED, _lib.EP_FULL, _lib.EP_BAG_EMPTY, _lib.EP_REFILLED)  # the steps whose atom belongs to the molecule
STATUS_NAMES = ('INACTIVE', 'PLACED', 'STOP', 'TOO_CLOSE', 'SOLO', 'FULL', 'BAG_EMPTY', 'ERROR', 'REFILLED', 'OUTSIDE')
BOND_COUNT = {1: 1, 5: 3, 6: 4, 7: 3, 8: 2, 9: 1}  # StochasticEnvironment.z_to_bond_count (environment.py:221-228)
MIN_FORMULA_VALIDITY = 0.25  # per try; 64 tries then all fail with probability 0.75^64 < 1e-7


@dataclass(eq=False)
class Episode:
    """one finished episode: the environment it ran in, the index of its (first) formula in `formulas`, the molecule (start
    structure first), the status that ended it (`_lib.EP_*`) and logp / v of each of its steps (the ending one included);
    `refills`: how often its bag was refilled; `bag`: the counts per `zs` entry of everything it was given (the first bag and
    every refill; with `size_range`, the formula drawn for it)"""
    env: int
    formula: int
    numbers: np.ndarray  # (n,) int64 atomic numbers
    positions: np.ndarray  # (n, 3) float64
    status: int
    logp: np.ndarray  # (steps,) float32
    v: np.ndarray  # (steps,) float32
    refills: int = 0
    bag: tuple = ()


def formula_to_bag(formula, zs: Sequence[int]) -> tuple:
    """counts per entry of `zs` of a formula in the reference's FormulaType, ((z, count), ...) (spaces.py:89-93)"""
    zs = list(zs)
    bag = [0] * len(zs)
    for z, count in formula:
        if z not in zs:
            raise ValueError(f'formula {formula}: atomic number {z} is not among zs {zs}')
        bag[zs.index(z)] += int(count)
    if bag[zs.index(0)] if 0 in zs else 0:
        raise ValueError(f'formula {formula} holds the null symbol')
    if sum(bag) <= 0:
        raise ValueError(f'formula {formula} is empty')
    return tuple(bag)


def formula_validity(bag, zs: Sequence[int], size_range) -> float:
    """Probability that one try of the formula draw is valid (environment.py:240-249): a formula of s symbols drawn with
    probability count / size has even bond parity iff its number of odd-bond symbols is even, (1 + (1 - 2q)^s) / 2 with q the
    total probability of the odd-bond elements; averaged over the sizes of [lo, hi) (hi alone when lo == hi)."""
    lo, hi = (int(x) for x in size_range)
    total = sum(int(c) for c in bag)
    q = sum(int(c) for c, z in zip(bag, zs) if c and BOND_COUNT[z] % 2) / total
    sizes = range(lo, hi) if lo < hi else [hi]
    return sum((1.0 + (1.0 - 2.0 * q)**s) / 2.0 for s in sizes) / len(sizes)


def scaffold_planes(canvas, zs: Sequence[int], scaffold_z: int) -> np.ndarray:
    """[P][4] float64 facets (outward unit normal, offset) of the convex hull of the atoms of element `scaffold_z` among the
    canvas items ((label, position), ...), `scipy.spatial.ConvexHull(...).equations`"""
    from scipy.spatial import ConvexHull, QhullError
    pts = np.array([xyz for label, xyz in canvas if zs[int(label)] == scaffold_z], dtype=np.float64).reshape(-1, 3)
    if len(pts) < 4:
        raise ValueError(f'the scaffold needs at least 4 atoms of element {scaffold_z}, the start structure holds {len(pts)}')
    try:
        planes = np.ascontiguousarray(ConvexHull(pts).equations, dtype=np.float64)
    except QhullError as e:
        raise ValueError(f'the {len(pts)} scaffold atoms span no volume (coplanar?): {str(e).splitlines()[0]}') from None
    if len(planes) > 2 * _lib.MG_MAX_CANVAS:
        raise ValueError(f'a scaffold hull of {len(planes)} facets (at most {2 * _lib.MG_MAX_CANVAS})')
    return planes


def check_rules(zs, bag_table, initial, num_refills, scaffold_z, hull_tol, size_range, max_formula_tries):
    """the host-side checks of DeviceEpisodes' rule keywords (no device needed); returns the scaffold planes or None"""
    zs = list(zs)
    if int(num_refills) < 0:
        raise ValueError(f'num_refills {num_refills} < 0')
    planes = None
    if scaffold_z is not None:
        if scaffold_z not in zs or scaffold_z == 0:
            raise ValueError(f'scaffold_z {scaffold_z} is not among zs {zs}')
        if not hull_tol >= 0.0:
            raise ValueError(f'hull_tol {hull_tol} is negative')
        if initial is None or not (len(initial) == 2 and isinstance(initial[0][0][0], (int, np.integer))):
            raise ValueError('scaffold_z needs ONE initial observation shared by all environments: the scaffold')
        if bag_table[:, zs.index(scaffold_z)].any():
            raise ValueError(f'a formula holds the scaffold element {scaffold_z}: a placed atom of it would join the hull in the '
                             'reference (environment.py:156-157), and the hull here is fixed')
        planes = scaffold_planes(initial[0], zs, scaffold_z)
    if size_range is not None:
        lo, hi = (int(x) for x in size_range)
        if len(bag_table) != 1:
            raise ValueError(f'size_range draws from exactly one formula, {len(bag_table)} were given')
        if int(num_refills) > 0:
            raise ValueError('size_range excludes refills (StochasticEnvironment has none)')
        if not 1 <= lo <= hi <= 255:
            raise ValueError(f'size_range {tuple(size_range)}: 1 <= lo <= hi <= 255')
        if not 1 <= int(max_formula_tries) <= 64:
            raise ValueError(f'max_formula_tries {max_formula_tries} outside 1..64')
        missing = [z for z, c in zip(zs, bag_table[0]) if c and z not in BOND_COUNT]
        if missing:
            raise ValueError(f'elements {missing} of the formula have no bond count ({sorted(BOND_COUNT)} have)')
        p = formula_validity(bag_table[0], zs, (lo, hi))
        if p < MIN_FORMULA_VALIDITY:
            raise ValueError(f'a formula drawn from {tuple(int(c) for c in bag_table[0])} with sizes {(lo, hi)} is valid (even bond '
                             f'parity) with probability {p:.3f} per try, below {MIN_FORMULA_VALIDITY}')
    return planes


class DeviceEpisodes:
    """`num_envs` environments with the rules of the reference's `MolecularEnvironment`, resident on the device of `ac`
    (CovariantAC or SchNetAC; training mode draws, evaluation mode takes the argmax variants).

    `formulas`: list of FormulaType, ((z, count), ...); every environment cycles through them on its own, episode k using
    `formulas[k % len(formulas)]` (environment.py:134-140).  `initial`: an observation, or one per environment, whose canvas is
    the structure every episode starts from (its bag is not used: bags come from `formulas`); None: empty canvases.

    The rules of the other environment classes (module docstring); with none of these keywords the step is `mg_episode_step`,
    with any of them `mg_episode_step_rules`:
    `num_refills` > 0: an empty bag is refilled that many times per episode; refills and resets advance ONE formula cycle
    (environment.py:185,196,206).  `scaffold_z`: new atoms must lie inside the convex hull of the atoms of that element in
    the ONE `initial` observation (at least 4, not coplanar), within `hull_tol` of its facets; the hull is fixed, so formulas
    holding `scaffold_z` are refused.  `size_range` = (lo, hi): `formulas` is one formula, and every episode's bag is drawn
    from it -- a size in [lo, hi) (hi when lo == hi), symbols with probability count / size, redrawn until the bond parity is
    even, at most `max_formula_tries` times (environment.py:232-249); `formula_seed` keys the draws of episode 0, the seed of
    the step that ends an episode those of the next.

    `shard` = (rank, world): `num_envs`, `formulas` and a per-environment `initial` list stay GLOBAL; the instance holds the
    environments `[lo, hi)` of `rollout.shard_bounds(num_envs, rank, world)` (`E` rows; `num_envs` keeps the global count).  Local
    row b is global environment `lo + b`: it draws from that environment's random streams -- actions and formulas -- and
    `Episode.env` and the rows handed to a reward function carry the global number.  None: (0, 1), everything."""

    def __init__(self, ac, formulas, num_envs: int, initial=None, min_atomic_distance: float = 0.6, max_solo_distance: float = 2.0,
                 num_refills: int = 0, scaffold_z: Optional[int] = None, hull_tol: float = 0.0, size_range=None, formula_seed: int = 0,
                 max_formula_tries: int = 64, shard=None):
        if num_envs < 1 or len(formulas) < 1:
            raise ValueError('DeviceEpisodes needs at least one environment and one formula')
        from .rollout import shard_bounds
        self.shard = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
        self.num_envs = int(num_envs)
        self.lo, self.hi = shard_bounds(self.num_envs, *self.shard)
        self.zs, self.N = list(ac.zs), ac.observation_space.canvas_space.size
        self.bag_table = np.array([formula_to_bag(f, self.zs) for f in formulas], dtype=np.int64)  # (F, Z)
        planes = check_rules(self.zs, self.bag_table, initial, num_refills, scaffold_z, hull_tol, size_range, max_formula_tries)
        if ac.theta.device.type != 'cuda':
            raise RuntimeError('DeviceEpisodes runs on the HIP device only (no CPU fallback)')
        self.ac, self.E = ac, self.hi - self.lo
        self.cols = ac.action_cols  # SchNetAC's 7-column rows / CovariantAC's (focus, element, d, x, y, z)
        self.min_atomic_distance, self.max_solo_distance = float(min_atomic_distance), float(max_solo_distance)
        self.num_refills, self.hull_tol = int(num_refills), float(hull_tol)
        self.size_range = None if size_range is None else (int(size_range[0]), int(size_range[1]))
        self.formula_seed, self.max_formula_tries = int(formula_seed), int(max_formula_tries)
        # the rule set beyond MolecularEnvironment's: None keeps the step on mg_episode_step
        self.rules = (self.num_refills > 0 or planes is not None or self.size_range is not None) or None
        empty = ((0, (0.0, 0.0, 0.0)), ) * self.N
        if initial is None:
            canvases = [empty] * self.E
        elif len(initial) == 2 and isinstance(initial[0][0][0], (int, np.integer)):
            canvases = [initial[0]] * self.E  # one observation
        else:
            canvases = [obs[0] for obs in initial]
            if len(canvases) != self.num_envs:
                raise ValueError(f'{len(canvases)} initial observations for {self.num_envs} environments')
            canvases = canvases[self.lo:self.hi]
        bag0 = tuple(int(c) for c in self.bag_table[0])
        self.canvas = ac.make_canvas([(tuple(c), bag0) for c in canvases])
        cv, dev = self.canvas, ac.theta.device
        if int(cv.natoms.max()) >= self.N:
            raise ValueError('an initial structure fills the canvas: there is nothing to place')
        self._start = (cv.pos64.clone(), cv.charges.clone(), cv.natoms_dev.clone())
        self._start_natoms = cv.natoms.copy()
        host64, hostz = cv.pos64.cpu().numpy(), cv.charges.cpu().numpy()
        self._start_atoms = [(hostz[e, :n].astype(np.int64), host64[e, :n].copy()) for e, n in enumerate(self._start_natoms)]
        self._formulas = torch.from_numpy(self.bag_table.astype(np.float32)).to(dev)
        self._zs_c = (C.c_int32 * len(self.zs))(*self.zs)
        self.planes = planes
        self._planes_dev = None if planes is None else torch.from_numpy(planes).to(dev)
        self.reset()

    def _rules_struct(self, seed: int) -> '_lib.EpisodeRules':
        r = _lib.EpisodeRules()
        r.num_refills, r.hull_tol = self.num_refills, self.hull_tol
        if self._planes_dev is not None:
            r.num_planes, r.planes = int(self._planes_dev.shape[0]), self._planes_dev.data_ptr()
        r.refills, r.formula_no = self.refills_dev.data_ptr(), self.formula_no_dev.data_ptr()
        if self.size_range is not None:
            r.stochastic, r.size_min, r.size_max, r.max_tries = 1, self.size_range[0], self.size_range[1], self.max_formula_tries
            r.seed, r.stream_base, r.stream_stride = int(seed) & 0xFFFFFFFFFFFFFFFF, self.lo, 1
            for i, c in enumerate(self.bag_table[0]):
                r.counts[i] = int(c)
        return r

    def reset(self) -> None:
        """every environment back to episode 0 on its start canvas; unfinished episodes are dropped"""
        cv, dev = self.canvas, self.ac.theta.device
        cv.pos64.copy_(self._start[0])
        cv.pos32.copy_(self._start[0].float())
        cv.charges.copy_(self._start[1])
        cv.natoms_dev.copy_(self._start[2])
        cv.bags.copy_(self._formulas[0].expand(self.E, -1))
        cv.natoms = self._start_natoms.copy()
        cv.bags_host = np.tile(self.bag_table[0], (self.E, 1))
        cv.last_placed = None
        self.alive = torch.ones(self.E, dtype=torch.int32, device=dev)
        self.episode_no_dev = torch.zeros(self.E, dtype=torch.int32, device=dev)
        self.episode_no = np.zeros(self.E, dtype=np.int64)  # host mirror
        self.alive_host = np.ones(self.E, dtype=bool)
        # position in the formula cycle and refills of the open episode (device arrays in rules mode only).  Refills advance the
        # cycle too; without them it IS the episode number, and the two mirrors are one array
        self.formula_no = np.zeros(self.E, dtype=np.int64) if self.num_refills > 0 else self.episode_no
        self.refills = np.zeros(self.E, dtype=np.int64)
        if self.rules:
            self.formula_no_dev = torch.zeros(self.E, dtype=torch.int32, device=dev)
            self.refills_dev = torch.zeros(self.E, dtype=torch.int32, device=dev)
        if self.size_range is not None:  # episode 0's formulas, drawn on the device like every later one
            ok = torch.empty(self.E, dtype=torch.int32, device=dev)
            rules = self._rules_struct(self.formula_seed)
            with self.ac._guard():
                _lib.check(_lib.lib().mg_episode_draw_formulas(self.E, len(self.zs), self._zs_c, C.byref(rules), _lib.ptr(cv.bags),
                                                               _lib.ptr(ok), self.ac._s()))
            if not bool(ok.cpu().numpy().all()):
                raise RuntimeError(f'no valid formula in {self.max_formula_tries} tries for some environment (formula_seed {self.formula_seed})')
            cv.bags_host = cv.bags.cpu().numpy().astype(np.int64)
        # everything the open episode was given so far, where that is not simply the bag of its formula
        self._given = cv.bags_host.copy() if self.num_refills > 0 or self.size_range is not None else None
        self._bag_tuples = [tuple(int(c) for c in bag) for bag in self.bag_table]
        self._open = [([], [], [], []) for _ in range(self.E)]  # per environment: numbers, positions, logp, v of the open episode
        self._last_launch = None

    def _sample(self, seed, acts, out, newpos, err) -> None:
        """the sampling launch on the resident canvases for either agent, keyed by (seed, lo + row): action rows -> `acts`,
        logp / ent / v -> `out`; SchNetAC's also places (`newpos`) and flags a disagreeing mirror in `err`, CovariantAC's
        leaves its launch in `_last_launch` for `_check_last_launch`"""
        if self.cols == 6:
            self._last_launch = self.ac._sample_canvas(self.canvas, seed, (self.lo, 1), acts, out)
        else:
            self.ac._sample_canvas(self.canvas, seed, (self.lo, 1), acts, newpos, out, err)

    def _mirror_disagrees(self) -> None:
        """`err[0]` of SchNetAC's `_sample` was set (CovariantAC's launch has no such flag: `_check_last_launch`)"""
        self.alive_host[:] = False
        raise RuntimeError('molgym_hip error -1: the device canvases disagree with the host mirror of the atom counts; '
                           'these episodes cannot go on (reset())')

    def _check_last_launch(self) -> None:
        """the list build of CovariantAC's sampling launches flags canvases that disagree with the host mirror in the workspace"""
        if self._last_launch is not None:
            self.ac.check_launch(self._last_launch)

    def _mirror_end(self, rows: np.ndarray, bags=None) -> None:
        """The ONE host mirror of the device's `ep_end_episode`, for the environments `rows` (indices) whose episode a step or a
        cut ended: the start's atom counts, the next episode, the next position of the formula cycle with no refills taken, the
        next bag -- `bags` (len(rows), Z) where the device drew them (`size_range`), the cycle's otherwise -- and nothing given
        or open but that bag."""
        cv = self.canvas
        cv.natoms[rows] = self._start_natoms[rows]
        self.episode_no[rows] += 1
        if self.num_refills > 0:  # (otherwise formula_no IS episode_no)
            self.formula_no[rows] += 1
            self.refills[rows] = 0
        cv.bags_host[rows] = self.bag_table[self.formula_no[rows] % len(self.bag_table)] if bags is None else bags
        if self._given is not None:
            self._given[rows] = cv.bags_host[rows]
        for e in rows.tolist():
            self._open[e] = ([], [], [], [])

    def step(self, seed: Optional[int] = None, hooks=None) -> dict:
        """One step of every environment: one sampling launch on the resident canvases, keyed as `step_canvas` keys it (row b
        reads the random stream (seed, lo + b), `lo` the first environment of the shard; `seed=None` draws `ac.draw_seed()`), then `mg_episode_step` (or
        `mg_episode_step_rules`, see the class).  No action lists, no distribution block, no cloned canvases.

        ONE small device-to-host copy per step remains, the record: status, element, newpos, logp / ent / v (and SchNetAC's
        mirror flag), 44 bytes per environment; with `size_range` also the bags, 4 bytes per symbol, for the rows that drew a
        new one.  The host needs the statuses at once, not only at the end: the next sampling launch is sized (`cfg.TA` /
        `cfg.TE`) from the host mirror of the atom counts (`canvas.natoms`), and that mirror follows from which rows placed an
        atom and which were reset.

        Returns dict(status (E,) int32, element (E,) int32, newpos (E, 3) float64, logp / v (E,) float32 CPU tensors,
        episodes: the `Episode`s this step finished, by environment).  A row with status ERROR raises RuntimeError, as the
        reference's `remove_atom_from_formula` does.

        `hooks` (molgym_amd/rollout.py): a pair of callables issued on the stream between the launches, `hooks[0](acts, out)`
        behind the sampling launch and `hooks[1](status, element, newpos)`, the device arrays of the step record, behind the
        episode step; None: nothing is added."""
        ac, cv, E = self.ac, self.canvas, self.E
        dev = ac.theta.device
        Z, F = len(self.zs), len(self.bag_table)
        sampled = self.size_range is not None
        o_out, o_st, o_el, o_err = 24 * E, 36 * E, 40 * E, 44 * E
        o_bag = o_err + 8
        rec = torch.empty(o_bag + (4 * E * Z if sampled else 0), dtype=torch.uint8, device=dev)
        newpos = rec[:o_out].view(torch.float64).view(E, 3)
        out = rec[o_out:o_st].view(torch.float32).view(3, E)
        status, element, err = rec[o_st:o_el].view(torch.int32), rec[o_el:o_err].view(torch.int32), rec[o_err:o_bag].view(torch.int32)
        acts = torch.empty(E, self.cols, dtype=torch.float32, device=dev)
        if self.rules and seed is None:
            seed = ac.draw_seed()  # (what the sampling launch would draw: the formula draws are keyed by the same seed)
        self._sample(seed, acts, out, newpos, err)
        if hooks is not None:
            hooks[0](acts, out)
        p = _lib.ptr
        with ac._guard():
            args = (E, self.N, Z, F, self.cols, 1 if self.cols == 6 else 0, self._zs_c, self.min_atomic_distance, self.max_solo_distance,
                    p(acts), p(newpos), p(cv.pos64), p(cv.pos32), p(cv.charges), p(cv.bags), p(cv.natoms_dev), p(self.alive),
                    p(self.episode_no_dev), p(self._start[0]), p(self._start[1]), p(self._start[2]), p(self._formulas), p(status),
                    p(element))
            if self.rules:
                rules = self._rules_struct(seed)
                _lib.check(_lib.lib().mg_episode_step_rules(*args, C.byref(rules), ac._s()))
                if sampled:
                    rec[o_bag:].view(torch.float32).view(E, Z).copy_(cv.bags)  # (device to device: still one copy to the host)
            else:
                _lib.check(_lib.lib().mg_episode_step(*args, ac._s()))
        if hooks is not None:
            hooks[1](status, element, newpos)
        host = rec.cpu().numpy()  # the one copy of the step
        if self.cols == 7 and int(host[o_err:o_err + 4].view(np.int32)[0]):
            self._mirror_disagrees()
        h_pos = host[:o_out].view(np.float64).reshape(E, 3).copy()
        h_out = host[o_out:o_st].view(np.float32).reshape(3, E).copy()
        h_st, h_el = host[o_st:o_el].view(np.int32).copy(), host[o_el:o_err].view(np.int32).copy()
        # the mirrors the next launch is sized from
        refilling = self.num_refills > 0
        placed = h_st == _lib.EP_PLACED
        if refilling:
            refilled = h_st == _lib.EP_REFILLED
            placed = placed | refilled
        done = np.nonzero(np.isin(h_st, DONE_STATUSES))[0]
        cv.natoms[placed] += 1
        cv.bags_host[np.nonzero(placed)[0], h_el[placed]] -= 1
        if refilling and refilled.any():  # environment.py:194-197: the next formula of the one cycle
            self.formula_no[refilled] += 1
            self.refills[refilled] += 1
            cv.bags_host[refilled] = self.bag_table[self.formula_no[refilled] % F]
            self._given[refilled] += cv.bags_host[refilled]
        finished = []
        for e in range(E):
            s = int(h_st[e])
            if s in (_lib.EP_INACTIVE, _lib.EP_ERROR):
                continue
            numbers, positions, logp, v = self._open[e]
            logp.append(h_out[0, e])
            v.append(h_out[2, e])
            if s in ATOM_STATUSES:
                numbers.append(self.zs[int(h_el[e])])
                positions.append(h_pos[e])
            if s != _lib.EP_PLACED and s != _lib.EP_REFILLED:
                z0, p0 = self._start_atoms[e]
                k = int(self.refills[e]) if refilling else 0
                f = int((self.formula_no[e] - k) % F)  # (the formula the episode began with)
                finished.append(Episode(env=self.lo + e, formula=f,
                                        numbers=np.concatenate([z0, np.array(numbers, dtype=np.int64)]),
                                        positions=np.concatenate([p0, np.array(positions, dtype=np.float64).reshape(-1, 3)]),
                                        status=s, logp=np.array(logp, dtype=np.float32), v=np.array(v, dtype=np.float32),
                                        refills=k, bag=self._bag_tuples[f] if self._given is None else tuple(self._given[e].tolist())))
        self._mirror_end(done, host[o_bag:].view(np.float32).reshape(E, Z)[done].astype(np.int64) if sampled else None)
        bad = np.nonzero(h_st == _lib.EP_ERROR)[0]
        self.alive_host[bad] = False
        if len(bad):
            e = int(bad[0])
            raise RuntimeError(f'environment {self.lo + e}: element index {int(h_el[e])} is out of range or not in its bag '
                               f'{tuple(int(c) for c in cv.bags_host[e])}' +
                               (f', or no valid formula was drawn in {self.max_formula_tries} tries' if sampled else '') +
                               f' ({len(bad)} environments stopped)')
        return {'status': h_st, 'element': h_el, 'newpos': h_pos, 'logp': torch.from_numpy(h_out[0].copy()),
                'v': torch.from_numpy(h_out[2].copy()), 'episodes': finished}

    def run(self, num_steps: Optional[int] = None, num_episodes: Optional[int] = None, seed: Optional[int] = None) -> List[Episode]:
        """Step until `num_steps` steps were taken or `num_episodes` episodes finished, whichever comes first, and return the
        finished episodes in the order of the step record: by step, then by environment (with `num_episodes`, exactly the
        first that many).  `seed`: the per-step seeds are drawn from a generator seeded with it, so equal seeds from equal
        states (`reset()`) give equal lists; None: every step draws `ac.draw_seed()`.  Episodes still open when the run ends stay
        open for the next call."""
        if num_steps is None and num_episodes is None:
            raise ValueError('run() needs num_steps or num_episodes')
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        episodes, steps = [], 0
        while (num_steps is None or steps < num_steps) and (num_episodes is None or len(episodes) < num_episodes):
            s = None if gen is None else int(torch.randint(0, 2**62, (1, ), generator=gen).item())
            episodes.extend(self.step(s)['episodes'])
            steps += 1
        self._check_last_launch()
        return episodes if num_episodes is None else episodes[:num_episodes]


def sample_molecules(ac, formulas, num_molecules: int, num_envs: Optional[int] = None, seed: Optional[int] = None, **kw) -> List[Episode]:
    """`num_molecules` finished episodes of `ac` over `formulas`, from `num_envs` device-resident environments (default: one
    per molecule, at most 256); further keywords go to `DeviceEpisodes`"""
    if num_envs is None:
        num_envs = max(1, min(int(num_molecules), 256))
    return DeviceEpisodes(ac, formulas, num_envs, **kw).run(num_episodes=int(num_molecules), seed=seed)
