"""Device rollouts: the trajectories of device-resident episodes recorded in HBM and handed to `ppo.train`.

`DeviceEpisodes` (molgym_amd/episodes.py) steps the reference's environments on the device, for sampling.  Training went the
long way round: `ppo._rollout_serial` runs Python environments, a `PPOBufferContainer.store` loop per row, uploads rewards and
values after the rollout and has `CovariantAC.prepare_rollout` parse every observation tuple again -- to upload what the
canvases held in HBM all along.  `DeviceRollout` keeps it there (for SchNetAC on request: `train_data(on_device=True)`).  Per step, between the sampling launch and the episode step,
`mg_traj_record` copies every row's canvas, bag, action row and logp / v into its slot of the store; behind the episode step
`mg_traj_status` adds the status and the rule reward.  After the last step one value-only sampling launch gives the bootstrap
values, `mg_traj_gae` evaluates every path of the store and `mg_adv_normalize` standardises (include/molgym_hip.h).

Sample order: environment e's step t of a T-step collect is sample e * T + t -- the order `PPOBufferContainer.merge()`
produces, since every live environment yields one sample per step (resets are immediate).  The store's arrays ARE the members
of `RolloutOnDevice`; nothing is transposed, compacted or parsed.

Rewards (environment.py:49-79): STOP pays 0.0 and an invalid action `min_reward`, written on the device.  A placed atom pays
`reward_fn(before, new_z, new_pos, rows)` -- called on the host, once per step, for the rows that placed one -- or 0.0 without a
reward function.  A reward below `min_reward` becomes `min_reward` and ends the episode: `mg_episode_cut` resets those rows
(status LOW_REWARD) before the next sampling launch, by the device function the step's own terminal branch calls; on the host
both ends go through `DeviceEpisodes._mirror_end`.  With `size_range` a reset needs a formula draw, which the cut does not
have: `reward_fn` together with `size_range` is refused.

`reward=PairReward(...)` (molgym_amd/rewards.py) pays a placed atom on the device instead: `mg_traj_pair_reward`, behind
`mg_traj_status`, reads the before-canvas from the slot the record kernel wrote, writes the reward and the cut flags, and
`mg_episode_cut` runs on those flags.  Nothing is uploaded; one copy of 12 bytes per environment brings reward and flag to the
host mirrors.  `reward_fn=PairReward(...).host` is the same reward by the host path.

Data parallelism: `DeviceRollout(..., shard=(rank, world))` records this rank's contiguous share of `num_envs` global environments
(`shard_bounds`); row b is global environment lo + b and draws from its streams.  `train_data()` then exchanges the stores in ONE
collective: `mg_traj_pack` -> a block of twelve 256-aligned sections (`exchange_layout`), `all_gather_blocks`, `mg_traj_unpack` ->
a gathered store in sample order g * T + t, `mg_adv_normalize` over all of it.  Every rank ends up with the bytes one process
driving all the environments with these seeds would hold (profiles/dp_device_rollout.md: where that was established)."""
import ctypes as C
import time
from typing import Optional

import numpy as np
import torch

from . import _lib
from .episodes import ATOM_STATUSES, DONE_STATUSES, STATUS_NAMES as EPISODE_STATUS_NAMES, DeviceEpisodes
from .observations import CarriedRollout

# the names of every status a store can hold (episodes.STATUS_NAMES plus the cut)
STATUS_NAMES = EPISODE_STATUS_NAMES + ('LOW_REWARD', )
END_STATUSES = DONE_STATUSES + (_lib.EP_LOW_REWARD, )  # the statuses that end an episode, and so a path of the rollout
MAX_STORE_ELEMENTS = 2**31  # E * capacity * N * 3 stays below it (mg_traj_record)
_ALIGN = 256
# the arrays of the store in the order they lie in it: name, dtype, elements per sample as a function of (N, Z, cols)
_FIELDS = (('pos64', torch.float64, lambda N, Z, c: 3 * N), ('logp', torch.float64, lambda N, Z, c: 1),
           ('val', torch.float64, lambda N, Z, c: 1), ('rew', torch.float64, lambda N, Z, c: 1),
           ('adv', torch.float64, lambda N, Z, c: 1), ('ret', torch.float64, lambda N, Z, c: 1),
           ('pos', torch.float32, lambda N, Z, c: 3 * N), ('charges', torch.int32, lambda N, Z, c: N),
           ('bags', torch.float32, lambda N, Z, c: Z), ('actions', torch.float32, lambda N, Z, c: c),
           ('status', torch.int32, lambda N, Z, c: 1))


def _layout(fields, S: int, canvas_size: int, num_zs: int, cols: int):
    """({name: (byte offset, dtype, elements per sample)}, total bytes) of `S` samples of `fields`, every array starting at a
    multiple of 256 bytes"""
    per = [k(canvas_size, num_zs, cols) for _, _, k in fields]
    nbytes = [S * k * (8 if dtype == torch.float64 else 4) for (_, dtype, _), k in zip(fields, per)]
    offs, total = _lib.sections(nbytes, _ALIGN)
    return {name: (off, dtype, k) for (name, dtype, _), k, off in zip(fields, per, offs)}, total


def store_layout(num_envs: int, capacity: int, canvas_size: int, num_zs: int, cols: int):
    """({name: (byte offset, dtype, elements per sample)}, total bytes) of a store of `num_envs * capacity` samples; every
    array starts at a multiple of 256 bytes"""
    return _layout(_FIELDS, int(num_envs) * int(capacity), canvas_size, num_zs, cols)


def shard_bounds(num_envs: int, rank: int, world: int):
    """(lo, hi): the contiguous share of `num_envs` environments that rank `rank` of `world` holds -- the split of
    `ppo._shard_global_config`: shares differ by at most one environment and every environment belongs to exactly one rank"""
    num_envs, rank, world = int(num_envs), int(rank), int(world)
    if world < 1:
        raise ValueError(f'world {world} < 1')
    if not 0 <= rank < world:
        raise ValueError(f'rank {rank} outside 0..{world - 1}')
    if num_envs < world:
        raise ValueError(f'{num_envs} environments cannot be dealt to {world} ranks')
    return (rank * num_envs) // world, ((rank + 1) * num_envs) // world


def exchange_layout(num_envs: int, world: int, T: int, canvas_size: int, num_zs: int, cols: int):
    """({name: (byte offset, dtype, elements per sample)}, block_bytes) of the block a rank sends when the stores of a `T`-step
    collect are exchanged (`mg_traj_pack` / `mg_traj_unpack`, include/molgym_hip.h): the arrays of the store in `_FIELDS` order,
    then `natoms`, the int32 atom counts of the samples.  Every section starts at a multiple of 256 bytes and is sized for the
    largest share, ceil(num_envs / world) * T samples, so the blocks of all ranks have the same byte count."""
    shard_bounds(num_envs, 0, world)
    S = (int(num_envs) + int(world) - 1) // int(world) * int(T)
    return _layout(_FIELDS + (('natoms', torch.int32, lambda N, Z, c: 1), ), S, canvas_size, num_zs, cols)


def all_gather_blocks(block: torch.Tensor) -> torch.Tensor:
    """[world * block_bytes] uint8 on the device of `block`: the equally sized blocks of all ranks in rank order, by ONE
    collective -- `all_gather_into_tensor` on the device for nccl, through host copies for gloo, which has no device all-gather
    (the two routes of `ppo._DeviceRunner.fold_rows`).  Without torch.distributed: `block` itself."""
    from . import ppo
    dist, rank, world = ppo._dist()
    if dist is None or world == 1:
        return block.reshape(-1)
    if ppo._comm_device(dist).type == 'cuda' and block.device.type == 'cuda':
        gathered = torch.empty(world * block.numel(), dtype=block.dtype, device=block.device)
        dist.all_gather_into_tensor(gathered, block.reshape(-1))
        return gathered
    host = block.reshape(-1).cpu()
    parts = [torch.empty_like(host) for _ in range(world)]
    dist.all_gather(parts, host)
    return torch.cat(parts).to(block.device)


def check_rollout_args(num_envs, capacity, canvas_size, reward_fn, size_range, reward=None, zs=None) -> None:
    """the host-side refusals of DeviceRollout's own arguments (no device needed); `zs`: the agent's element list, which a
    device `reward` must have been built for"""
    if int(capacity) < 1:
        raise ValueError(f'capacity {capacity} < 1: it is the largest num_steps of one collect')
    if int(num_envs) * int(capacity) * int(canvas_size) * 3 >= MAX_STORE_ELEMENTS:
        raise ValueError(f'a store of {num_envs} environments x {capacity} steps x {canvas_size} atoms x 3 holds 2^31 elements or more')
    if reward_fn is not None and size_range is not None:
        raise ValueError('reward_fn together with size_range: a reward below min_reward cuts the episode, and the reset of a cut '
                         'row would need a formula draw on the device (size_range with reward_fn=None works: nothing is cut)')
    if reward is not None:
        if reward_fn is not None:
            raise ValueError('reward together with reward_fn: a placed atom is paid by one of them (reward_fn=reward.host is the '
                             'host path of the same reward)')
        if size_range is not None:
            raise ValueError('reward together with size_range: a reward below min_reward cuts the episode, and the reset of a cut '
                             'row would need a formula draw on the device')
        if zs is not None and [int(z) for z in reward.zs] != [int(z) for z in zs]:
            raise ValueError(f'reward was built for zs {list(reward.zs)}, the agent has {list(zs)}')


def check_on_device(on_device) -> Optional[bool]:
    """`train_data`'s keyword: None (the agent's default form), True or False -- nothing that merely converts to one"""
    if on_device is not None and not isinstance(on_device, (bool, np.bool_)):
        raise ValueError(f'on_device {on_device!r}: None (the agent\'s default), True (a rollout that stays on the device) or '
                         'False (the host form of data())')
    return None if on_device is None else bool(on_device)


def check_num_steps(num_steps, capacity) -> int:
    if not 1 <= int(num_steps) <= int(capacity):
        raise ValueError(f'num_steps {num_steps} outside 1..capacity ({capacity})')
    return int(num_steps)


def reference_reward(obj):
    """`reward_fn` from an object with the reference's `calculate(atoms, new_atom) -> (reward, info)` (reward.py); `ase` is
    imported when the function is called, not before"""

    def reward_fn(before, new_z, new_pos, rows):
        from ase import Atom, Atoms
        out = np.empty(len(rows), dtype=np.float64)
        for k, (numbers, positions) in enumerate(before):
            atoms = Atoms(numbers=[int(z) for z in numbers], positions=np.asarray(positions, dtype=np.float64).reshape(-1, 3))
            out[k] = obj.calculate(atoms, Atom(int(new_z[k]), position=tuple(float(x) for x in new_pos[k])))[0]
        return out

    return reward_fn


def discounted_returns(status: np.ndarray, rew: np.ndarray, gamma: float) -> np.ndarray:
    """(E, T) float64 returns-to-go of the rewards `rew` (E, T) within the episodes the statuses `status` delimit, bootstrap 0:
    `discount_cumsum` of `DynamicPPOBuffer.finish_path`, one float64 operation at a time, for all environments at once (the
    tail of a row that is still open is not an episode: its entries are not returns)"""
    E, T = status.shape
    ends = np.isin(status, END_STATUSES)
    ret, run = np.zeros((E, T), dtype=np.float64), np.zeros(E, dtype=np.float64)
    for t in range(T - 1, -1, -1):
        run = np.where(ends[:, t], 0.0, run)
        run = rew[:, t] + gamma * run
        ret[:, t] = run
    return ret


def episode_statistics(status: np.ndarray, ret: np.ndarray):
    """(returns, lengths) of the episodes that ENDED in a store with statuses `status` (E, T) and returns-to-go `ret` (E, T), in
    the order `PPOBufferContainer` records them: by step, then by environment.  A path runs from the slot behind the previous
    ending (or slot 0) to its ending slot; its return is `ret` at its first slot."""
    E, T = status.shape
    ends = np.isin(status, END_STATUSES)
    last = np.maximum.accumulate(np.where(ends, np.arange(T)[None, :], -1), axis=1)  # the latest ending slot up to t
    start = np.concatenate([np.zeros((E, 1), dtype=np.int64), last[:, :-1] + 1], axis=1)  # the first slot of the path t is in
    tt, ee = np.nonzero(ends.T)
    return ret[ee, start[ee, tt]], tt - start[ee, tt] + 1


class _Views:
    """typed views of the first `num_envs * T` samples of every array of a store"""

    def __init__(self, store: torch.Tensor, table: dict, S: int):
        for name, (off, dtype, k) in table.items():
            size = 8 if dtype == torch.float64 else 4
            setattr(self, name, store[off:off + S * k * size].view(dtype))


class DeviceRollout(DeviceEpisodes):
    """`DeviceEpisodes` that record their trajectories in a store on the device (module docstring).

    `capacity`: the largest `num_steps` of one `collect`; `gamma`, `lam`: GAE's; `min_reward`: what an invalid action pays and
    the reward below which an episode is cut; `reward_fn(before, new_z, new_pos, rows) -> float64 (len(rows),)`: the reward of
    the atoms placed in one step -- `before` the list of (numbers, positions) of those rows' molecules without the new atom,
    `new_z` / `new_pos` the atoms, `rows` their environments -- or None: a placed atom pays 0.0.  `reward`: a
    `rewards.PairReward` built for the agent's `zs`, evaluated on the device (module docstring); not together with `reward_fn`
    or `size_range`.  `store`: a uint8 device tensor
    of exactly `store_bytes` bytes to record into (default: allocated here).  Further keywords go to `DeviceEpisodes`;
    `reward_fn` together with `size_range` raises ValueError.

    Episodes still open when a collect ends stay open: the next collect continues them, and their first path there starts at
    slot 0.  `reset()` drops them.

    `shard=(rank, world)` (a `DeviceEpisodes` keyword): the instance records this rank's share of `num_envs` global
    environments in a store of its own, `collect()` communicates nothing and leaves the RAW advantages in the store at
    `world > 1`, and `train_data()` is a collective that hands every rank the rollout of all environments (module functions
    `shard_bounds`, `exchange_layout`, `all_gather_blocks`)."""

    def __init__(self, ac, formulas, num_envs: int, capacity: int, gamma: float = 0.99, lam: float = 0.95, min_reward: float = -0.6,
                 reward_fn=None, store: Optional[torch.Tensor] = None, reward=None, **device_episode_keywords):
        N = ac.observation_space.canvas_space.size
        shard = device_episode_keywords.get('shard') or (0, 1)
        lo, hi = shard_bounds(num_envs, *shard)
        check_rollout_args(hi - lo, capacity, N, reward_fn, device_episode_keywords.get('size_range'), reward, ac.zs)
        if int(num_envs) * int(capacity) * int(N) * 3 >= MAX_STORE_ELEMENTS:  # a second time: the store train_data() gathers
            raise ValueError(f'a gathered store of {num_envs} environments x {capacity} steps x {N} atoms x 3 holds 2^31 elements or more')
        self.capacity, self.gamma, self.lam, self.min_reward = int(capacity), float(gamma), float(lam), float(min_reward)
        self.reward_fn, self.reward = reward_fn, reward
        self._T = 0
        self._block = self._gstore = None  # the send block of `pack`, the gathered store of `unpack_gathered`
        super().__init__(ac, formulas, num_envs, **device_episode_keywords)
        self._table, self.store_bytes = store_layout(self.E, self.capacity, self.N, len(self.zs), self.cols)
        dev = ac.theta.device
        if store is None:
            store = torch.zeros(self.store_bytes, dtype=torch.uint8, device=dev)
        if store.dtype != torch.uint8 or store.numel() != self.store_bytes or store.device != dev or not store.is_contiguous() or \
                store.data_ptr() % 16:
            raise ValueError(f'store: a contiguous, 16-byte aligned uint8 tensor of exactly {self.store_bytes} bytes on {dev}')
        self.store = store
        self._last_val = torch.zeros(self.E, dtype=torch.float64, device=dev)
        # per environment: episodes that ended, sum and sum of squares of their lengths (mg_traj_gae)
        self._len_stats = torch.zeros(2, self.E, dtype=torch.float64, device=dev)
        self._num_done = torch.zeros(self.E, dtype=torch.int32, device=dev)
        if reward is not None:
            # the atom counts before the step, and what the step paid: [reward f64 | cut flag i32] per environment, ONE copy
            self._natoms_before = torch.zeros(self.E, dtype=torch.int32, device=dev)
            self._paid = torch.zeros(12 * self.E, dtype=torch.uint8, device=dev)
            self._reward_tables = reward.device_tables(dev)

    def reset(self) -> None:
        """every environment back to episode 0 on its start canvas; the store holds no rollout any more"""
        super().reset()
        self._T = 0
        self._natoms_hist = self._status_hist = self._episode_stats = self._gathered = None

    def _views(self, T: Optional[int] = None) -> _Views:
        return _Views(self.store, self._table, self.E * (self._T if T is None else T))

    # ---- one step ------------------------------------------------------------------------------------------------------------
    def _hooks(self, t: int, T: int, v: _Views):
        ac, cv, E, p = self.ac, self.canvas, self.E, _lib.ptr

        def record(acts, out):
            with ac._guard():
                _lib.check(_lib.lib().mg_traj_record(E, T, t, self.N, len(self.zs), self.cols, p(cv.pos32), p(cv.pos64), p(cv.charges),
                                                     p(cv.bags), p(acts), p(out), p(self.alive), p(v.pos), p(v.pos64), p(v.charges),
                                                     p(v.bags), p(v.actions), p(v.logp), p(v.val), ac._s()))

        def status(st, element=None, newpos=None):
            with ac._guard():
                _lib.check(_lib.lib().mg_traj_status(E, T, t, p(st), self.min_reward, p(v.status), p(v.rew), ac._s()))

        if self.reward is None:
            return record, status
        R, (four_eps, sigma2) = self.reward, self._reward_tables
        reward_out, flags = self._paid[:8 * E].view(torch.float64), self._paid[8 * E:].view(torch.int32)

        def record_counts(acts, out):
            record(acts, out)
            with ac._guard():
                self._natoms_before.copy_(cv.natoms_dev)  # (device to device: the count the reward kernel walks the slot with)

        def status_reward_cut(st, element, newpos):
            status(st)
            with ac._guard():
                _lib.check(_lib.lib().mg_traj_pair_reward(E, T, t, self.N, len(self.zs), self._zs_c, p(four_eps), p(sigma2),
                                                          R.distance_penalty, R.cutoff2, self.min_reward, p(st),
                                                          p(element), p(newpos), p(self._natoms_before), p(self.alive),
                                                          p(v.pos64), p(v.charges), p(v.rew), p(reward_out), p(flags), ac._s()))
            self._cut_flagged(t, T, v, flags)

        return record_counts, status_reward_cut

    def _cut(self, t: int, T: int, v: _Views, flags: np.ndarray) -> None:
        """mg_episode_cut for the rows with flags != 0 (a host array: uploaded)"""
        self._cut_flagged(t, T, v, torch.from_numpy(np.ascontiguousarray(flags, dtype=np.int32)).to(self.ac.theta.device))

    def _cut_flagged(self, t: int, T: int, v: _Views, d_flags: torch.Tensor) -> None:
        """mg_episode_cut for the rows whose entry of the int32 device array `d_flags` is not 0"""
        ac, cv, p = self.ac, self.canvas, _lib.ptr
        rules = (p(self.refills_dev), p(self.formula_no_dev)) if self.rules else (None, None)
        with ac._guard():
            _lib.check(_lib.lib().mg_episode_cut(self.E, self.N, len(self.zs), len(self.bag_table), T, t, p(d_flags), self.min_reward,
                                                 p(cv.pos64), p(cv.pos32), p(cv.charges), p(cv.bags), p(cv.natoms_dev), p(self.alive),
                                                 p(self.episode_no_dev), p(self._start[0]), p(self._start[1]), p(self._start[2]),
                                                 p(self._formulas), rules[0], rules[1], p(v.status), p(v.rew), ac._s()))

    def _pay(self, t: int, T: int, v: _Views, rec: dict, st: np.ndarray, before_open) -> None:
        """the caller's rewards of step t into the store, and the cut of the rows whose reward is below min_reward; `st`, the
        host statuses of the step, and the host mirrors follow the cut.  Returns (rows, their rewards as the store holds them),
        or None when no row placed an atom."""
        rows = np.nonzero(np.isin(st, ATOM_STATUSES))[0]
        if len(rows) == 0:
            return None
        before = []
        for e in rows:
            numbers, positions, n = before_open[e]
            z0, p0 = self._start_atoms[e]
            before.append((np.concatenate([z0, np.array(numbers[:n], dtype=np.int64)]),
                           np.concatenate([p0, np.array(positions[:n], dtype=np.float64).reshape(-1, 3)])))
        new_z = np.array([self.zs[int(el)] for el in rec['element'][rows]], dtype=np.int64)
        r = np.asarray(self.reward_fn(before, new_z, rec['newpos'][rows].copy(), rows + self.lo), dtype=np.float64).reshape(-1)
        if len(r) != len(rows):
            raise ValueError(f'reward_fn returned {len(r)} rewards for {len(rows)} rows')
        # ONE upload, 16 bytes per row: [slot | reward] as float64 (slots are exact in it)
        buf = torch.from_numpy(np.stack([(rows * T + t).astype(np.float64), r])).to(self.ac.theta.device)
        v.rew.index_copy_(0, buf[0].long(), buf[1])
        low = r < self.min_reward
        if low.any():
            flags = np.zeros(self.E, dtype=np.int32)
            flags[rows[low]] = 1
            self._cut(t, T, v, flags)
        self._mirror_cut(st, rows, low)
        return rows, np.where(low, self.min_reward, r)

    def _paid_on_device(self, st: np.ndarray):
        """`_pay` for `reward=`: the status hook has paid and cut on the device already; ONE copy, 12 bytes per environment,
        brings the rewards and the cut flags the host mirrors need"""
        rows = np.nonzero(np.isin(st, ATOM_STATUSES))[0]
        if len(rows) == 0:
            return None
        host, E = self._paid.cpu().numpy(), self.E
        r, low = host[:8 * E].view(np.float64)[rows], host[8 * E:].view(np.int32)[rows] != 0
        self._mirror_cut(st, rows, low)
        return rows, np.where(low, self.min_reward, r)

    def _mirror_cut(self, st: np.ndarray, rows: np.ndarray, low: np.ndarray) -> None:
        """the host mirrors behind mg_episode_cut: of `rows`, the atom-placing rows of a step with statuses `st`, those with
        `low` were paid min_reward, and where the step had left the episode open it ended (`st` <- LOW_REWARD)"""
        cut = rows[low & ((st[rows] == _lib.EP_PLACED) | (st[rows] == _lib.EP_REFILLED))]  # the others had ended already
        st[cut] = _lib.EP_LOW_REWARD
        self._mirror_end(cut)

    # ---- a rollout -----------------------------------------------------------------------------------------------------------
    def collect(self, num_steps: int, seed: Optional[int] = None) -> dict:
        """`num_steps` steps of every environment into the store, then the bootstrap values, GAE and the standardised
        advantages (at `world > 1` the raw ones: `train_data()` standardises over the gathered rollout; no communication here,
        and the statistics returned are this rank's -- `global_statistics` has those of all ranks).  The seeds are drawn as `ppo._rollout_serial` draws them -- one per step and one more for the value-only
        launch behind the last step (the launch `step_canvas(canvas, commit=False)` issues; nothing of it is copied to the
        host), from `ac.draw_seed()`, or from a generator seeded with `seed`.  Returns the keys of `ppo.batch_rollout`: time,
        return_mean / return_std / episode_length_mean / episode_length_std over the episodes that ended (NaN when none did),
        as `PPOBufferContainer` records them."""
        T = check_num_steps(num_steps, self.capacity)
        start_time = time.time()
        ac, cv, E = self.ac, self.canvas, self.E
        dev = ac.theta.device
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        draw = ac.draw_seed if gen is None else (lambda: int(torch.randint(0, 2**62, (1, ), generator=gen).item()))
        self._T = 0  # (a collect that raises leaves no rollout behind)
        self._gathered = None
        v = self._views(T)
        natoms_hist, status_hist = np.empty((E, T), dtype=np.int32), np.empty((E, T), dtype=np.int32)
        rew_hist = np.zeros((E, T), dtype=np.float64)  # host mirror of the rewards: the episodic returns need no copy back
        invalid = (_lib.EP_TOO_CLOSE, _lib.EP_SOLO, _lib.EP_OUTSIDE)
        for t in range(T):
            natoms_hist[:, t] = cv.natoms
            before_open = [(o[0], o[1], len(o[0])) for o in self._open] if self.reward_fn is not None else None
            rec = self.step(draw(), hooks=self._hooks(t, T, v))
            st = rec['status']
            rew_hist[np.isin(st, invalid), t] = self.min_reward
            if self.reward_fn is not None:
                paid = self._pay(t, T, v, rec, st, before_open)
            elif self.reward is not None:
                paid = self._paid_on_device(st)
            else:
                paid = None
            if paid is not None:
                rew_hist[paid[0], t] = paid[1]
            status_hist[:, t] = st
        # the bootstrap values: one more sampling launch on the canvases as they stand, nothing committed
        acts = torch.empty(E, self.cols, dtype=torch.float32, device=dev)
        out = torch.empty(3, E, dtype=torch.float32, device=dev)
        err = torch.zeros(2, dtype=torch.int32, device=dev) if self.cols == 7 else None
        self._sample(draw(), acts, out, torch.empty(E, 3, dtype=torch.float64, device=dev), err)
        self._last_val.copy_(out[2])
        p = _lib.ptr
        with ac._guard():
            _lib.check(_lib.lib().mg_traj_gae(E, T, p(v.status), p(v.rew), p(v.val), p(self._last_val), self.gamma, self.lam, p(v.adv),
                                              p(v.ret), p(self._num_done), p(self._len_stats[0]), p(self._len_stats[1]), ac._s()))
            if self.shard[1] == 1:  # (a shard keeps the raw advantages: the standardisation is over the merged rollout)
                _lib.check(_lib.lib().mg_adv_normalize(E * T, p(v.adv), None, ac._s()))
        # ONE small copy for the statistics: the length sums and the counts per environment (and SchNetAC's mirror flag)
        tail = [self._len_stats.reshape(-1), self._num_done.double()] + ([] if err is None else [err.double()])
        host = torch.cat(tail).cpu().numpy()
        if err is not None and int(host[-2]):
            self._mirror_disagrees()
        self._check_last_launch()  # as DeviceEpisodes.run(): the list build's flags of the last launch
        # the episodic returns: float64 on the host from the mirrored rewards, as DynamicPPOBuffer.finish_path forms them
        returns, lengths = episode_statistics(status_hist, discounted_returns(status_hist, rew_hist, self.gamma))
        n = int(host[2 * E:3 * E].sum())
        len_sum, len_sq = host[:E].sum(), host[E:2 * E].sum()  # (sums of small integers: exact)
        if n != len(lengths) or len_sum != lengths.sum() or len_sq != (lengths * lengths).sum():
            raise RuntimeError(f'the store holds {n} finished episodes of {len_sum} steps, the host mirror of the statuses '
                               f'{len(lengths)} of {lengths.sum()}')
        self._T, self._natoms_hist, self._status_hist = T, natoms_hist, status_hist
        self._episode_stats = (returns, lengths)
        nan = float('nan')
        return {
            'time': time.time() - start_time,
            'return_mean': np.mean(returns).item() if n else nan,
            'return_std': np.std(returns).item() if n else nan,
            'episode_length_mean': float(len_sum / n) if n else nan,
            'episode_length_std': np.std(lengths).item() if n else nan,
        }

    def statuses(self) -> np.ndarray:
        """(E, T) int32: the status of every sample of the last collect (`STATUS_NAMES`), from the host mirror"""
        self._need_rollout()
        return self._status_hist.copy()

    def _need_rollout(self) -> None:
        if self._T < 1:
            raise RuntimeError('the store holds no rollout: collect() first')

    def global_statistics(self, info: dict) -> dict:
        """`info` (what `collect` returned) with the episode statistics over the rollouts of ALL ranks: the (return, length) rows
        of the episodes that ended travel through `ppo.all_gather_rows`, as `ppo._global_rollout_info` gathers a container's.  A
        collective call under torch.distributed (every rank makes it; rank 0 logs from it); without it, `info`."""
        from . import ppo
        self._need_rollout()
        dist, rank, world = ppo._dist()
        if dist is None:
            return info
        returns, lengths = self._episode_stats
        full = ppo.all_gather_rows(np.stack([np.asarray(returns, dtype=np.float64), np.asarray(lengths, dtype=np.float64)], axis=1).reshape(-1, 2))
        out = dict(info)
        if len(full):
            out.update(return_mean=np.mean(full[:, 0]).item(), return_std=np.std(full[:, 0]).item(),
                       episode_length_mean=np.mean(full[:, 1]).item(), episode_length_std=np.std(full[:, 1]).item())
        return out

    # ---- the exchange under data parallelism ---------------------------------------------------------------------------------
    def _exchange_args(self, T: int):
        """(sections, block_bytes, sec_off, sec_words as ctypes arrays) of a T-step exchange"""
        sections, block_bytes = exchange_layout(self.num_envs, self.shard[1], T, self.N, len(self.zs), self.cols)
        n = len(sections)
        off = (C.c_int64 * n)(*[o for o, _, _ in sections.values()])
        words = (C.c_int32 * n)(*[k * (2 if dtype == torch.float64 else 1) for _, dtype, k in sections.values()])
        return sections, block_bytes, off, words

    def pack(self) -> torch.Tensor:
        """this rank's send block of the last collect (`exchange_layout`; one `mg_traj_pack`, one upload of the atom counts): a
        uint8 device tensor of `block_bytes`, owned by the instance and written again by the next call.  It is zeroed when it is
        allocated, not per call."""
        self._need_rollout()
        ac, T = self.ac, self._T
        sections, block_bytes, off, words = self._exchange_args(T)
        block = self._block
        if block is None or block.numel() != block_bytes:
            block = self._block = torch.zeros(block_bytes, dtype=torch.uint8, device=ac.theta.device)
        v = self._views()
        natoms = torch.from_numpy(np.ascontiguousarray(self._natoms_hist.reshape(-1), dtype=np.int32)).to(ac.theta.device)
        arrays = (C.c_void_p * len(sections))(*[(natoms if name == 'natoms' else getattr(v, name)).data_ptr() for name in sections])
        with ac._guard():
            _lib.check(_lib.lib().mg_traj_pack(self.num_envs, self.shard[1], self.shard[0], T, self.capacity, self.N, len(sections), off,
                                               words, arrays, _lib.ptr(block), block_bytes, ac._s()))
        return block

    def unpack_gathered(self, blocks: torch.Tensor, T: Optional[int] = None, on_device: Optional[bool] = None) -> dict:
        """`train_data()` behind the collective: `blocks`, the send blocks of all ranks of a `T`-step collect in rank order
        ([world * block_bytes] uint8 on the device; `T` defaults to the last collect's), go into a gathered store of `num_envs`
        environments by ONE `mg_traj_unpack`; `mg_adv_normalize` standardises its `num_envs * T` advantages and one
        device-to-host copy brings the gathered atom counts.  The result is kept until the next collect or reset."""
        on_device = check_on_device(on_device)
        ac, dev = self.ac, self.ac.theta.device
        T = check_num_steps(self._T if T is None else T, self.capacity)
        world = self.shard[1]
        sections, block_bytes, off, words = self._exchange_args(T)
        if blocks.dtype != torch.uint8 or blocks.numel() != world * block_bytes or blocks.device != dev or not blocks.is_contiguous():
            raise ValueError(f'blocks: a contiguous uint8 tensor of {world} x {block_bytes} bytes on {dev}')
        if self._gstore is None:
            self._gtable, nbytes = store_layout(self.num_envs, self.capacity, self.N, len(self.zs), self.cols)
            self._gstore = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        S = self.num_envs * T
        v = _Views(self._gstore, self._gtable, S)
        natoms = torch.empty(S, dtype=torch.int32, device=dev)
        arrays = (C.c_void_p * len(sections))(*[(natoms if name == 'natoms' else getattr(v, name)).data_ptr() for name in sections])
        with ac._guard():
            _lib.check(_lib.lib().mg_traj_unpack(self.num_envs, world, T, self.capacity, self.N, len(sections), off, words,
                                                 _lib.ptr(blocks), block_bytes, arrays, ac._s()))
            _lib.check(_lib.lib().mg_adv_normalize(S, _lib.ptr(v.adv), None, ac._s()))
        self._gathered = (T, natoms.cpu().numpy())
        return self._form(v, self._gathered[1], S, on_device, world)

    def _form(self, v: _Views, natoms: np.ndarray, S: int, on_device: Optional[bool], world: int) -> dict:
        """the rollout of `S` samples in the views `v`, with the host mirror `natoms` of its atom counts, as `train_data` hands it out"""
        if on_device is None:
            on_device = self.cols != 7
        if not on_device:
            return self._host_form(v, natoms, S)
        N = self.N
        if self.cols == 7:
            from .agents.internal import IntRolloutOnDevice
            rollout = IntRolloutOnDevice.from_store(self.ac, natoms, v.pos64, v.charges, v.bags, v.actions, v.logp, v.adv, v.ret)
        else:
            from .agents.covariant import RolloutOnDevice
            rollout = RolloutOnDevice(self.ac, natoms, v.pos.view(S, N, 3), v.charges.view(S, N), v.bags.view(S, len(self.zs)),
                                      v.actions.view(S, self.cols), v.logp, v.adv, v.ret)
        obs = CarriedRollout(S, rollout)
        obs.world = world
        return dict(obs=obs, act=v.actions.view(S, self.cols), ret=v.ret, adv=v.adv, logp=v.logp)

    def train_data(self, on_device: Optional[bool] = None) -> dict:
        """What `ppo.train` takes as `data`.  On the device: `obs` is a `CarriedRollout` -- `len` is the number of samples, and the
        agent's `prepare_rollout` returns the prepared rollout it carries, whose members are views of the store -- and act / ret
        / adv / logp are device tensors, views of the store too: the next collect overwrites them.  CovariantAC carries a
        `RolloutOnDevice` (a mini-batch is one `mg_gather_rows`), SchNetAC an `IntRolloutOnDevice` (a mini-batch is one
        `mg_int_gather_batch`: the ragged 3B-molecule batch and both z-matrix placements of every row, assembled on the device).
        `on_device`: None -- CovariantAC's rollout stays on the device, SchNetAC gets the host form, `data()`, whose mini-batches
        `IntRollout` assembles on the host; True -- the device form for either agent; False -- `data()`.

        With `shard=(rank, world)`, `world > 1`, this is a COLLECTIVE call: every rank must make it.  `pack()`, ONE all-gather of
        the blocks (`all_gather_blocks`), then `unpack_gathered`: every rank then holds the same bytes, the rollout of all
        `num_envs` environments in the sample order g * T + t, with the advantages standardised over all of it, in the same forms
        (the host form is that of the gathered store).  `obs.world` is the world it was gathered over, which `ppo.train` asks
        for.  The result is kept until the next `collect` or `reset`: a second call does not communicate."""
        on_device = check_on_device(on_device)
        self._need_rollout()
        world = self.shard[1]
        if world == 1:
            return self._form(self._views(), self._natoms_hist.reshape(-1), self.E * self._T, on_device, 1)
        if self._gathered is None:
            return self.unpack_gathered(all_gather_blocks(self.pack()), self._T, on_device)
        T, natoms = self._gathered
        return self._form(_Views(self._gstore, self._gtable, self.num_envs * T), natoms, self.num_envs * T, on_device, world)

    def data(self) -> dict:
        """The reference's host form of the rollout, for both agents: `obs` the list of observation tuples, rebuilt from the
        float64 canvases, the charges and the bags of the store (ONE device-to-host copy per rollout), `act` a float32 array;
        adv / ret / logp stay device tensors (float64 views of the store), as `DynamicPPOBuffer.get_data(device=...)` leaves
        them.  On a shard this is the rank's own share (its advantages raw at `world > 1`)."""
        self._need_rollout()
        return self._host_form(self._views(), self._natoms_hist.reshape(-1), self.E * self._T)

    def _host_form(self, v: _Views, natoms: np.ndarray, S: int) -> dict:
        N, Z = self.N, len(self.zs)
        packed = torch.cat([v.pos64, v.charges.double(), v.bags.double(), v.actions.double()]).cpu().numpy()
        pos = packed[:3 * S * N].reshape(S, N, 3)
        charges = np.rint(packed[3 * S * N:4 * S * N]).astype(np.int64).reshape(S, N)
        bags = np.rint(packed[4 * S * N:4 * S * N + S * Z]).astype(np.int64).reshape(S, Z)
        act = packed[4 * S * N + S * Z:].astype(np.float32).reshape(S, self.cols)
        label_of = {int(z): i for i, z in enumerate(self.zs)}
        null = (0, (0.0, 0.0, 0.0))
        obs = []
        for s in range(S):
            n = int(natoms[s])
            xyz = pos[s, :n].tolist()
            canvas = tuple((label_of[int(z)], (q[0], q[1], q[2])) for z, q in zip(charges[s, :n], xyz)) + (null, ) * (N - n)
            obs.append((canvas, tuple(int(c) for c in bags[s])))
        return dict(obs=obs, act=act, ret=v.ret, adv=v.adv, logp=v.logp)
