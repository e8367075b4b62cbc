"""Rewards a device rollout can pay without leaving the device.

The reference's rewards (`InteractionReward`, `SolvationReward`, reward.py) are -(E(all) - E(before) - E(atom)) from a quantum
chemistry code, which cannot run on the device.  For a pairwise-additive potential that energy difference is exactly the sum of
the pair terms between the new atom and the atoms already there -- a reduction over one canvas row, which `DeviceRollout` holds
in HBM.  `PairReward` is that reward for a 12-6 Lennard-Jones potential, with `SolvationReward`'s distance penalty
(reward.py:92-94): `DeviceRollout(reward=PairReward(...))` evaluates it in `mg_traj_pair_reward` (include/molgym_hip.h), and
`PairReward.host` is the float64 mirror with the signature of `reward_fn`.  No element parameters are shipped: the caller
supplies them.

The operation order is the interface; the kernel and the mirror state the same one, in float64 without contraction, from the
same table bytes.  Placing element a at q next to atoms j = 0 .. n-1 (element b_j at p_j, in canvas slot order):

    d = q - p_j;  r2 = (dx*dx + dy*dy) + dz*dz;  V_j = 0.0 if a cutoff is given and r2 > cutoff*cutoff, else
    s = sigma2[a][b_j] / r2;  s3 = (s*s)*s;  V_j = four_eps[a][b_j] * (s3*s3 - s3)
    dE = ((V_0 + V_1) + V_2) + ...                sequential in slot order, 0.0 for n = 0
    pen = distance_penalty * sqrt((qx*qx + qy*qy) + qz*qz)
    reward = -(dE + pen);  a NaN reward becomes -inf

Coincident atoms give r2 = 0 and inf - inf = NaN, so -inf: below any `min_reward`, the step pays `min_reward` and the episode is
cut."""
from typing import Optional, Sequence

import numpy as np

from . import _lib


class PairReward:
    """12-6 Lennard-Jones interaction of a placed atom with the atoms before it, minus `distance_penalty * |position|`.

    `zs`: the agent's element list.  `epsilon`, `sigma`: per-element sequences in `zs` order, mixed once in float64 --
    sigma_ij = (sigma_i + sigma_j) / 2, eps_ij = sqrt(eps_i * eps_j) -- or full symmetric [Z][Z] tables.  `cutoff`: pairs with
    r2 > cutoff^2 contribute nothing (None: every pair counts).  The tables kept are `four_eps` = 4 eps_ij and `sigma2` =
    sigma_ij^2, [Z][Z] float64; the kernel reads an upload of exactly these bytes.  ValueError: non-finite or negative entries,
    asymmetric tables, len(zs) outside 2..MG_MAX_Z, a negative or non-finite distance_penalty, cutoff <= 0."""

    def __init__(self, zs: Sequence[int], epsilon, sigma, distance_penalty: float = 0.0, cutoff: Optional[float] = None):
        self.zs = [int(z) for z in zs]
        Z = len(self.zs)
        if not 2 <= Z <= _lib.MG_MAX_Z:
            raise ValueError(f'{Z} elements: len(zs) must lie in 2..{_lib.MG_MAX_Z}')
        eps = self._table('epsilon', epsilon, Z, lambda a, b: np.sqrt(a * b))
        sig = self._table('sigma', sigma, Z, lambda a, b: (a + b) / 2.0)
        self.eps, self.sigma = eps, sig
        self.four_eps = np.ascontiguousarray(4.0 * eps)
        self.sigma2 = np.ascontiguousarray(sig * sig)
        if not (np.isfinite(self.four_eps).all() and np.isfinite(self.sigma2).all()):
            raise ValueError('4 * epsilon or sigma^2 overflows float64')
        self.distance_penalty = float(distance_penalty)
        if not (np.isfinite(self.distance_penalty) and self.distance_penalty >= 0.0):
            raise ValueError(f'distance_penalty {distance_penalty} is negative or not finite')
        if cutoff is not None and not float(cutoff) > 0.0:
            raise ValueError(f'cutoff {cutoff} <= 0')
        self.cutoff = None if cutoff is None else float(cutoff)
        # what r2 is compared against: +inf compares as "no cutoff" does
        self.cutoff2 = float('inf') if cutoff is None else float(np.float64(self.cutoff) * np.float64(self.cutoff))
        self._device_tables = {}

    @staticmethod
    def _table(name, values, Z, mix) -> np.ndarray:
        t = np.asarray(values, dtype=np.float64)
        if t.shape not in ((Z, ), (Z, Z)):
            raise ValueError(f'{name}: {Z} per-element values in zs order, or a [{Z}][{Z}] table (got shape {t.shape})')
        if not np.isfinite(t).all() or (t < 0.0).any():
            raise ValueError(f'{name} holds a negative or non-finite entry')
        if t.ndim == 1:
            t = mix(t[:, None], t[None, :])
        if not np.array_equal(t, t.T):
            raise ValueError(f'{name}: the [{Z}][{Z}] table is not symmetric')
        return np.ascontiguousarray(t, dtype=np.float64)

    def device_tables(self, device):
        """(four_eps, sigma2) on `device`: uploaded once per device, the bytes of the host tables"""
        import torch
        key = str(device)
        if key not in self._device_tables:
            self._device_tables[key] = (torch.from_numpy(self.four_eps).to(device), torch.from_numpy(self.sigma2).to(device))
        return self._device_tables[key]

    def pair(self, a: int, b: int, r2):
        """V of one pair of table row `a` and column `b` at squared distance `r2` (np.float64)"""
        if r2 > self.cutoff2:
            return np.float64(0.0)
        s = self.sigma2[a, b] / r2
        s3 = (s * s) * s
        return self.four_eps[a, b] * (s3 * s3 - s3)

    def reward(self, numbers, positions, new_z: int, q) -> float:
        """the reward of placing element `new_z` at `q` next to the atoms (`numbers`, `positions`), in their order"""
        a = self.zs.index(int(new_z))
        q = np.asarray(q, dtype=np.float64).reshape(3)
        positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        with np.errstate(all='ignore'):
            dE = np.float64(0.0)
            for j, z in enumerate(numbers):  # an explicit fold: np.sum is pairwise
                p = positions[j]
                dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
                V = self.pair(a, self.zs.index(int(z)), (dx * dx + dy * dy) + dz * dz)
                dE = V if j == 0 else dE + V
            pen = np.float64(self.distance_penalty) * np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
            r = -(dE + pen)
        return float('-inf') if np.isnan(r) else float(r)

    def energy_forces(self, numbers, positions, fixed=None):
        """(E, grad (n, 3), gmax) of one whole molecule under this potential, without `distance_penalty` (it belongs to a
        placement, not to a structure): the float64 mirror of `mg_pair_energy_forces`, in the order molgym_amd/relax.py states.
        `fixed`: a boolean mask or atom indices; those atoms' gradient is +0.0."""
        from . import relax
        return relax.energy_forces(self, numbers, positions, fixed)

    def host(self, before, new_z, new_pos, rows) -> np.ndarray:
        """`reward_fn` of `DeviceRollout`: the float64 mirror of `mg_traj_pair_reward`"""
        out = np.empty(len(rows), dtype=np.float64)
        for k, (numbers, positions) in enumerate(before):
            out[k] = self.reward(numbers, positions, new_z[k], new_pos[k])
        return out
