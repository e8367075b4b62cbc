"""Device-resident episodes: sample whole molecules from a policy without host environments.

A trained policy is a generative model, and sampling from it needs no reward: energies are computed afterwards on the
finished structures.  `batch_rollout` over Python environments pays, per environment and step, an `ase.Atoms`, an
observation tuple of `canvas_size` items, a re-upload of every canvas that ended and a reward call whose result is thrown
away -- all around a policy step of a fraction of a millisecond.  Here the canvases stay in HBM (`agents/canvas.py`) and
the environment's rules run there too: one sampling launch (`_sample_canvas`, the launch `step_canvas` issues) and one
`mg_episode_step` (include/molgym_hip.h) per step apply the two distance rules, the bag decrement, the terminal test and
the reset of finished environments of the reference's `MolecularEnvironment` (environment.py:49-118,134-140).

Not covered, by design (there is no reward on the device): `min_reward` termination, `ConstrainedMolecularEnvironment`'s
hull test, refills, `StochasticEnvironment`'s formula sampling, data-parallel sharding (one process, one device)."""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

DONE_STATUSES = (_lib.EP_STOP, _lib.EP_TOO_CLOSE, _lib.EP_SOLO, _lib.EP_FULL, _lib.EP_BAG_EMPTY)
ATOM_STATUSES = (_lib.EP_PLACED, _lib.EP_FULL, _lib.EP_BAG_EMPTY)  # the steps whose atom belongs to the molecule
STATUS_NAMES = ('INACTIVE', 'PLACED', 'STOP', 'TOO_CLOSE', 'SOLO', 'FULL', 'BAG_EMPTY', 'ERROR')


@dataclass(eq=False)
class Episode:
    """one finished episode: the environment it ran in, the index of its formula in `formulas`, the molecule (start structure
    first), the status that ended it (`_lib.EP_*`) and logp / v of each of its steps (the ending one included)"""
    env: int
    formula: int
    numbers: np.ndarray  # (n,) int64 atomic numbers
    positions: np.ndarray  # (n, 3) float64
    status: int
    logp: np.ndarray  # (steps,) float32
    v: np.ndarray  # (steps,) float32


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


class DeviceEpisodes:
    """`num_envs` environments with the rules of the reference's `MolecularEnvironment`, resident on the device of `ac`
    (CovariantAC or SchNetAC; training mode draws, evaluation mode takes the argmax variants).

    `formulas`: list of FormulaType, ((z, count), ...); every environment cycles through them on its own, episode k using
    `formulas[k % len(formulas)]` (environment.py:134-140).  `initial`: an observation, or one per environment, whose canvas is
    the structure every episode starts from (its bag is not used: bags come from `formulas`); None: empty canvases."""

    def __init__(self, ac, formulas, num_envs: int, initial=None, min_atomic_distance: float = 0.6, max_solo_distance: float = 2.0):
        if ac.theta.device.type != 'cuda':
            raise RuntimeError('DeviceEpisodes runs on the HIP device only (no CPU fallback)')
        if num_envs < 1 or len(formulas) < 1:
            raise ValueError('DeviceEpisodes needs at least one environment and one formula')
        self.ac, self.E = ac, int(num_envs)
        self.zs, self.N = list(ac.zs), ac.observation_space.canvas_space.size
        from .agents.internal import SchNetAC
        self.cols = 7 if isinstance(ac, SchNetAC) else 6  # SchNetAC's 7-column rows / CovariantAC's (focus, element, d, x, y, z)
        self.min_atomic_distance, self.max_solo_distance = float(min_atomic_distance), float(max_solo_distance)
        self.bag_table = np.array([formula_to_bag(f, self.zs) for f in formulas], dtype=np.int64)  # (F, Z)
        empty = ((0, (0.0, 0.0, 0.0)), ) * self.N
        if initial is None:
            canvases = [empty] * self.E
        elif len(initial) == 2 and isinstance(initial[0][0][0], (int, np.integer)):
            canvases = [initial[0]] * self.E  # one observation
        else:
            canvases = [obs[0] for obs in initial]
            if len(canvases) != self.E:
                raise ValueError(f'{len(canvases)} initial observations for {self.E} environments')
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
        self.reset()

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
        self._open = [([], [], [], []) for _ in range(self.E)]  # per environment: numbers, positions, logp, v of the open episode
        self._last_launch = None

    def step(self, seed: Optional[int] = None) -> dict:
        """One step of every environment: one sampling launch on the resident canvases, keyed as `step_canvas` keys it (row b
        reads the random stream (seed, b); `seed=None` draws `ac.draw_seed()`), then `mg_episode_step`.  No action lists, no
        distribution block, no cloned canvases.

        ONE small device-to-host copy per step remains, the record: status, element, newpos, logp / ent / v (and SchNetAC's
        mirror flag), 44 bytes per environment.  The host needs the statuses at once, not only at the end: the next sampling
        launch is sized (`cfg.TA` / `cfg.TE`) from the host mirror of the atom counts (`canvas.natoms`), and that mirror
        follows from which rows placed an atom and which were reset.

        Returns dict(status (E,) int32, element (E,) int32, newpos (E, 3) float64, logp / v (E,) float32 CPU tensors,
        episodes: the `Episode`s this step finished, by environment).  A row with status ERROR raises RuntimeError, as the
        reference's `remove_atom_from_formula` does."""
        ac, cv, E = self.ac, self.canvas, self.E
        dev = ac.theta.device
        o_out, o_st, o_el, o_err = 24 * E, 36 * E, 40 * E, 44 * E
        rec = torch.empty(o_err + 8, dtype=torch.uint8, device=dev)
        newpos = rec[:o_out].view(torch.float64).view(E, 3)
        out = rec[o_out:o_st].view(torch.float32).view(3, E)
        status, element, err = rec[o_st:o_el].view(torch.int32), rec[o_el:o_err].view(torch.int32), rec[o_err:].view(torch.int32)
        acts = torch.empty(E, self.cols, dtype=torch.float32, device=dev)
        if self.cols == 6:
            self._last_launch = ac._sample_canvas(cv, seed, (0, 1), acts, out)
        else:
            ac._sample_canvas(cv, seed, (0, 1), acts, newpos, out, err)
        p = lambda t: C.c_void_p(t.data_ptr())
        with ac._guard():
            _lib.check(_lib.lib().mg_episode_step(E, self.N, len(self.zs), len(self.bag_table), self.cols, 1 if self.cols == 6 else 0,
                                                  self._zs_c, self.min_atomic_distance, self.max_solo_distance, p(acts), p(newpos),
                                                  p(cv.pos64), p(cv.pos32), p(cv.charges), p(cv.bags), p(cv.natoms_dev), p(self.alive),
                                                  p(self.episode_no_dev), p(self._start[0]), p(self._start[1]), p(self._start[2]),
                                                  p(self._formulas), p(status), p(element), ac._s()))
        host = rec.cpu().numpy()  # the one copy of the step
        if self.cols == 7 and int(host[o_err:o_err + 4].view(np.int32)[0]):  # (CovariantAC's launch has no such flag: run() checks)
            self.alive_host[:] = False
            raise RuntimeError('molgym_hip error -1: the device canvases disagree with the host mirror of the atom counts; '
                               'these episodes cannot go on (reset())')
        h_pos = host[:o_out].view(np.float64).reshape(E, 3).copy()
        h_out = host[o_out:o_st].view(np.float32).reshape(3, E).copy()
        h_st, h_el = host[o_st:o_el].view(np.int32).copy(), host[o_el:o_err].view(np.int32).copy()
        # the mirrors the next launch is sized from
        placed = h_st == _lib.EP_PLACED
        done = np.isin(h_st, DONE_STATUSES)
        cv.natoms[placed] += 1
        cv.bags_host[np.nonzero(placed)[0], h_el[placed]] -= 1
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
            if s != _lib.EP_PLACED:
                z0, p0 = self._start_atoms[e]
                finished.append(Episode(env=e, formula=int(self.episode_no[e] % len(self.bag_table)),
                                        numbers=np.concatenate([z0, np.array(numbers, dtype=np.int64)]),
                                        positions=np.concatenate([p0, np.array(positions, dtype=np.float64).reshape(-1, 3)]),
                                        status=s, logp=np.array(logp, dtype=np.float32), v=np.array(v, dtype=np.float32)))
                self._open[e] = ([], [], [], [])
        self.episode_no[done] += 1
        cv.natoms[done] = self._start_natoms[done]
        cv.bags_host[done] = self.bag_table[self.episode_no[done] % len(self.bag_table)]
        bad = np.nonzero(h_st == _lib.EP_ERROR)[0]
        self.alive_host[bad] = False
        if len(bad):
            e = int(bad[0])
            raise RuntimeError(f'environment {e}: element index {int(h_el[e])} is out of range or not in its bag '
                               f'{tuple(int(c) for c in cv.bags_host[e])} ({len(bad)} environments stopped)')
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
        if self._last_launch is not None and hasattr(self.ac, 'check_inputs'):
            # the list build of the sampling launches flags canvases that disagree with the host mirror in the workspace
            self.ac.__dict__.setdefault('_unchecked', {})[0] = self._last_launch
            self.ac.check_inputs()
        return episodes if num_episodes is None else episodes[:num_episodes]


def sample_molecules(ac, formulas, num_molecules: int, num_envs: Optional[int] = None, seed: Optional[int] = None, **kw) -> List[Episode]:
    """`num_molecules` finished episodes of `ac` over `formulas`, from `num_envs` device-resident environments (default: one
    per molecule, at most 256); further keywords go to `DeviceEpisodes`"""
    if num_envs is None:
        num_envs = max(1, min(int(num_molecules), 256))
    return DeviceEpisodes(ac, formulas, num_envs, **kw).run(num_episodes=int(num_molecules), seed=seed)
