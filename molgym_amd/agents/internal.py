"""Internal-coordinate (SchNet) actor-critic on the gfx950 HIP kernels.

Drop-in for /root/reference/molgym/agents/internal/agent.py:17-353: same constructor keywords
(model_util.py:18-24), same ``step(observations, actions)`` contract with the 7-column action rows
``[stop, focus, element, distance, angle, dihedral, kappa]`` (agent.py:26,306-308).  The reference runs the
schnetpack SchNet embedding 3*B times per call at batch size 1 (agent.py:128,177); here the host builds ONE
ragged batch of 3B molecules -- the canvases and the canvases plus the hypothetical new atom at +/- dihedral,
placed by the z-matrix helper (internal/zmat.py:66-133, float64 numpy, no gradient, as in the reference which
goes through ``to_numpy``) -- and the whole step is two C-ABI calls.  ``step(observations)`` (rollouts) draws the
sub-actions stage by stage from the same kernels (see ``_step_sample``).
"""
import ctypes as C
import os
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib, layout
from .._lib import ptr
from ..observations import CarriedRollout, compact_canvases, observation_arrays
from ..spaces import ActionSpace, ObservationSpace, ObservationType
from .base import FlatThetaAgent, check_action_rows


def place_new_atoms(pos: np.ndarray, natoms: np.ndarray, focus: np.ndarray, distance, angle, dihedral) -> np.ndarray:
    """Vectorised zmat.position_atom_helper: pos (B, N, 3) float64 (real atoms first) -> new positions (B, 3)."""
    B, N, _ = pos.shape
    out = np.zeros((B, 3))
    if np.any((focus >= natoms) & (natoms > 0)) or np.any(focus < 0):
        raise RuntimeError('Focus greater than number of atoms')
    nz = np.nonzero(natoms > 0)[0]
    if len(nz) == 0:
        return out
    p, n, f = pos[nz], natoms[nz], focus[nz]
    fpos = p[np.arange(len(nz)), f]
    dist = np.sqrt(np.sum(np.square(p - fpos[:, None, :]), axis=-1))
    dist = np.where(np.arange(N)[None, :] < n[:, None], dist, np.inf)
    order = np.argsort(dist, axis=1, kind='stable')  # sorted() in the reference is stable too
    rows = np.arange(len(nz))
    p2 = p[rows, order[:, 0]]
    p1 = np.where((n >= 2)[:, None], p[rows, order[:, min(1, N - 1)]], p2 + np.array([1.0, 0.0, 0.0]))
    p0_three = p[rows, order[:, min(2, N - 1)]]
    p0 = np.where((n >= 3)[:, None], p0_three,
                  np.where((n == 2)[:, None], p2 + p1 + np.array([1.0, 1.0, 0.0]), p2 + np.array([0.0, 1.0, 0.0])))
    d, a, h = distance[nz, None], angle[nz, None], dihedral[nz, None]
    x, y, z = d * np.cos(a), d * np.cos(h) * np.sin(a), d * np.sin(h) * np.sin(a)
    v_a = p1 - p0
    v_b = p2 - p1
    v_b = v_b / np.linalg.norm(v_b, axis=1, keepdims=True)
    c_ab = np.cross(v_a, v_b)
    c_ab = c_ab / np.linalg.norm(c_ab, axis=1, keepdims=True)
    c_ab_b = np.cross(c_ab, v_b)
    out[nz] = p2 - v_b * x + c_ab_b * y + c_ab * z
    return out


class IntBatch:
    def __init__(self, cfg, mol_off, edge_off, molZ, molpos, bags, actions, logp=None, adv=None, ret=None):
        self.cfg, self.mol_off, self.edge_off, self.molZ, self.molpos = cfg, mol_off, edge_off, molZ, molpos
        self.bags, self.actions = bags, actions
        self.logp, self.adv, self.ret = logp, adv, ret


class IntRollout:
    """A rollout prepared for `ppo.train`'s device path.  The ragged 3B-molecule batch of a mini-batch depends on
    which samples are in it (z-matrix placement per sample, molecule / pair offsets), so it is assembled on the host
    per mini-batch; the float64 loss inputs are parked in HBM once and gathered on the device."""

    def __init__(self, ac, data):
        self.ac = ac
        # parsed ONCE for the whole rollout, together with the z-matrix placements of the recorded actions: a mini-batch is
        # then numpy slicing + the ragged assembly (the per-mini-batch parse + placement was 0.8 ms of host time)
        self.parsed = ac._parse(data['obs'])
        self.placed = ac._placements(self.parsed, np.asarray(data['act']))
        self.logp, self.adv, self.ret = ac._f64(data['logp']), ac._f64(data['adv']), ac._f64(data['ret'])

    def minibatch(self, indices: np.ndarray, idx_dev: Optional[torch.Tensor] = None) -> IntBatch:
        idx = np.asarray(indices, dtype=np.int64)
        batch = self.ac._assemble(tuple(x[idx] for x in self.parsed), tuple(x[idx] for x in self.placed))
        if idx_dev is None:
            idx_dev = torch.from_numpy(idx).to(self.logp.device)
        with self.ac._guard():
            batch.logp, batch.adv, batch.ret = _lib.gather_rows((self.logp, self.adv, self.ret), idx_dev, self.ac._s())
        return batch


def gather_totals(natoms) -> Tuple[int, int, int]:
    """(TA, MA, ME) of the 3B-molecule batch of samples with these atom counts, in int64: TA = sum n real atoms, MA = 3 TA + 2 B
    atoms with the two appended ones, ME = sum (3 n^2 + n) ordered pairs (n (n - 1) of the base molecule, (n + 1) n of each
    copy).  The kernels index pairs with 32 bits: ME >= 2^31 raises ValueError."""
    n = np.asarray(natoms, dtype=np.int64).reshape(-1)
    TA = int(n.sum())
    MA, ME = 3 * TA + 2 * len(n), int((3 * n * n + n).sum())
    if ME >= 2**31:
        raise ValueError(f'a mini-batch of {len(n)} samples with {TA} atoms has {ME} atom pairs: 2^31 or more')
    return TA, MA, ME


class IntRolloutOnDevice:
    """A rollout parked in HBM whose mini-batches are assembled there: `minibatch` is numpy on the host mirror of the atom counts
    for the totals, then ONE `mg_int_gather_batch` on the current stream into one packed device buffer -- offsets, atoms, both
    z-matrix placements of every recorded action row (mg_int_place's float64 arithmetic), bags, action rows and logp / adv / ret.
    Same `minibatch(indices, idx_dev=None) -> IntBatch` as `IntRollout`.

    What only the device can see -- its atom counts disagreeing with the mirror, an index outside the rollout -- is ORed into
    `err` by the launches, which then write a batch of zeros inside the sizes the host gave; `check()` reads the flag and raises."""

    def __init__(self, ac, natoms, pos64, charges, natoms_dev, bags, actions, logp, adv, ret):
        S, N, Z = len(natoms), ac.num_atoms, ac.num_zs
        dev = ac.theta.device
        self.ac, self.natoms, self.num_samples = ac, np.asarray(natoms, dtype=np.int64).reshape(-1), S
        want = ((pos64, torch.float64, S * N * 3), (charges, torch.int32, S * N), (natoms_dev, torch.int32, S),
                (bags, torch.float32, S * Z), (actions, torch.float32, S * 7), (logp, torch.float64, S), (adv, torch.float64, S),
                (ret, torch.float64, S))
        for t, dtype, numel in want:
            if t.dtype != dtype or t.numel() != numel or not t.is_contiguous() or t.device != dev:
                raise ValueError(f'a parked array of {t.numel()} {t.dtype} elements on {t.device} (contiguous: {t.is_contiguous()}) '
                                 f'where {numel} contiguous {dtype} on {dev} belong')
        self.t = tuple(t for t, _, _ in want)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._zs = (C.c_int32 * _lib.MG_MAX_Z)(*[int(z) for z in ac.zs])

    @classmethod
    def from_store(cls, ac, natoms, pos64, charges, bags, actions, logp, adv, ret) -> 'IntRolloutOnDevice':
        """the members are views of a `DeviceRollout` store (the next collect overwrites them); `natoms`, the host mirror of
        the atom counts that sizes every mini-batch, is uploaded once: the device's counts ARE the mirror"""
        natoms = np.ascontiguousarray(natoms, dtype=np.int32).reshape(-1)
        return cls(ac, natoms, pos64, charges, torch.from_numpy(natoms).to(ac.theta.device), bags, actions, logp, adv, ret)

    @classmethod
    def from_host(cls, ac, data) -> 'IntRolloutOnDevice':
        """the reference's host form of a rollout (`data['obs']` observation tuples, `data['act']` action rows): parsed once,
        ONE packed upload of positions, charges, atom counts, bags and action rows; logp / adv / ret as `IntRollout` takes them.
        The action rows' focus / element ranges are checked here, once, with the errors of the host placement."""
        charges, bags, natoms, pos64 = ac._parse(data['obs'])
        acts = check_action_rows(data['act'], len(natoms), 7, 1, 2, ac.num_atoms, ac.num_zs)
        if np.any((np.rint(acts[:, 1]) >= natoms) & (natoms > 0)):
            raise RuntimeError('Focus greater than number of atoms')
        pos_w = np.ascontiguousarray(pos64, dtype=np.float64).reshape(-1).view(np.int32)  # (4-byte words for the packed upload)
        d_pos, d_charges, d_natoms, d_bags, d_acts = ac._upload_packed(pos_w, np.ascontiguousarray(charges, dtype=np.int32),
                                                                      np.ascontiguousarray(natoms, dtype=np.int32),
                                                                      np.ascontiguousarray(bags, dtype=np.float32), acts)
        return cls(ac, natoms, d_pos.view(torch.float64), d_charges.reshape(-1), d_natoms, d_bags.reshape(-1), d_acts.reshape(-1),
                   *(ac._f64(data[k]).contiguous() for k in ('logp', 'adv', 'ret')))

    def minibatch(self, indices: np.ndarray, idx_dev: Optional[torch.Tensor] = None) -> IntBatch:
        ac = self.ac
        idx = np.asarray(indices, dtype=np.int64)
        B, N, Z = len(idx), ac.num_atoms, ac.num_zs
        cfg = ac._cfg(self.natoms[idx])
        MA, dev = cfg.MA, self.err.device
        if idx_dev is None:
            idx_dev = torch.from_numpy(idx).to(dev)
        # one allocation, every section a multiple of 16 bytes from its start: the three float64 columns, then the 4-byte arrays
        words = (6 * B, 3 * B + 1, 3 * B + 1, MA, 3 * MA, B * Z, 7 * B)
        offs, total = _lib.sections(words, 4)
        buf = torch.empty(total, dtype=torch.int32, device=dev)
        f64 = buf[:6 * B].view(torch.float64)
        logp, adv, ret = f64[:B], f64[B:2 * B], f64[2 * B:]
        mol_off, edge_off, molZ = (buf[o:o + w] for o, w in zip(offs[1:4], words[1:4]))
        molpos = buf[offs[4]:offs[4] + 3 * MA].view(torch.float32).view(MA, 3)
        bags = buf[offs[5]:offs[5] + B * Z].view(torch.float32).view(B, Z)
        actions = buf[offs[6]:offs[6] + 7 * B].view(torch.float32).view(B, 7)
        with ac._guard():
            _lib.check(_lib.lib().mg_int_gather_batch(B, N, Z, self.num_samples, cfg.TA, MA, cfg.ME, self._zs, ptr(idx_dev), *(ptr(t) for t in self.t),
                                                      ptr(mol_off), ptr(edge_off), ptr(molZ), ptr(molpos), ptr(bags), ptr(actions),
                                                      ptr(logp), ptr(adv), ptr(ret), ptr(self.err), ac._s()))
        return IntBatch(cfg, mol_off, edge_off, molZ, molpos, bags, actions, logp, adv, ret)

    def check(self) -> None:
        """raise if a gather so far saw what the host could not (reads the flag: call it where the stream is drained anyway)"""
        flag = int(self.err.item())
        if flag:
            raise RuntimeError(f'molgym_hip error -1: the parked rollout disagrees with the host mirror of its atom counts, or a '
                               f'mini-batch index lies outside it (flag {flag}); the mini-batches gathered from it held zeros')


class _IntStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, ac, batch):
        lib = _lib.lib()
        nbytes = C.c_size_t()
        _lib.check(lib.mg_int_workspace_bytes(C.byref(batch.cfg), C.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=theta.device)
        out = torch.empty(3, batch.cfg.B, dtype=torch.float32, device=theta.device)
        with torch.cuda.device(theta.device):
            _lib.check(lib.mg_int_forward(C.byref(batch.cfg), ptr(theta), ptr(batch.mol_off), ptr(batch.edge_off),
                                          ptr(batch.molZ), ptr(batch.molpos), ptr(batch.bags), ptr(batch.actions),
                                          ptr(ws), nbytes.value, ptr(out), ac._s()))
        ctx.save_for_backward(theta, ws)
        ctx.batch, ctx.ac = batch, ac
        ac._last_ws = ws
        return out

    @staticmethod
    def backward(ctx, gout):
        theta, ws = ctx.saved_tensors
        b = ctx.batch
        grad = torch.zeros_like(theta)
        gout = gout.contiguous()
        with torch.cuda.device(theta.device):
            _lib.check(_lib.lib().mg_int_backward(C.byref(b.cfg), ptr(theta), ptr(b.mol_off), ptr(b.edge_off),
                                                  ptr(b.molZ), ptr(b.molpos), ptr(b.bags), ptr(b.actions),
                                                  ptr(ws), ws.numel(), ptr(gout), ptr(grad), ctx.ac._s()))
        return grad, None, None


class SchNetAC(FlatThetaAgent):
    # batch_rollout samples on device-resident canvases (`step_canvas`) only when this is set: those draws come from the keyed
    # device streams, not from torch's RNG, so the numbers differ from `step(obs)` (same distributions).  A class attribute, so
    # that a whole-module pickle of an older version (no instance value) stays on `step(obs)`.
    rollout_on_canvas = False
    # prepare_rollout parks a host rollout in HBM and assembles its mini-batches there (`IntRolloutOnDevice.from_host`) only when
    # this is set; a class attribute for the same reason
    gather_on_device = False
    action_cols = 7  # (stop, focus, element, distance, angle, dihedral, kappa)
    # `_last_sample_cfg`: the batch sizes of the last `_sample_canvas`; `_draw_par_c`: the constants of `_draw_par`
    _TRANSIENT = FlatThetaAgent._TRANSIENT + (('_last_sample_cfg', None), ('_draw_par_c', None))

    def __init__(self, observation_space: ObservationSpace, action_space: ActionSpace,
                 min_max_distance: Tuple[float, float], network_width: int, device=None):
        super().__init__(observation_space, action_space)
        self.num_atoms = self.observation_space.canvas_space.size
        if not 1 <= self.num_atoms <= _lib.MG_MAX_CANVAS:
            raise RuntimeError(f'canvas_size {self.num_atoms}: the HIP kernels support canvases of 1..{_lib.MG_MAX_CANVAS} atoms '
                               f'(molecules of up to {_lib.MG_MAX_CANVAS + 1} atoms with the appended one)')
        if not 2 <= len(self.observation_space.zs) <= _lib.MG_MAX_Z:
            raise RuntimeError(f'len(zs) {len(self.observation_space.zs)}: the HIP kernels support element sets of '
                               f'2..{_lib.MG_MAX_Z} symbols')
        self.device = torch.device(device) if device is not None else torch.device('cuda')
        self.zs = list(self.observation_space.zs)
        self.num_zs = len(self.zs)
        self.network_width = network_width
        self.min_distance, self.max_distance = min_max_distance
        self.slot_table, total = layout.offsets_internal(self.num_zs, network_width)
        self.theta = torch.nn.Parameter(self._init_theta(total))
        self.rollout_on_canvas = os.environ.get('MG_INT_CANVAS_ROLLOUT') == '1'
        self.gather_on_device = os.environ.get('MG_INT_DEVICE_GATHER') == '1'
        self.to(self.device)

    def _init_theta(self, total: int) -> torch.Tensor:
        """schnetpack initialisers (Embedding N(0,1) with a zero padding row, Dense = xavier_uniform + zero
        bias), orthogonal MLPs with zero bias (modules.py:30-34), log stds of agent.py:69-70."""
        theta = torch.zeros(total)
        for name, (off, shape) in self.slot_table.items():
            n = int(np.prod(shape))
            view = theta[off:off + n].view(shape)
            if name == 'embedding_fn.embedding.weight':
                view.normal_()
                view[0].zero_()
            elif name.startswith('embedding_fn') and name.endswith('weight'):
                torch.nn.init.xavier_uniform_(view)
            elif name == 'log_stds':
                view.copy_(torch.log(torch.tensor([0.15, 0.25, 0.25])))
            elif name.endswith('weight'):
                torch.nn.init.orthogonal_(view)
            # every bias starts at zero
        return theta

    def _parse(self, observations: List[ObservationType]):
        """What make_batch needs from the observations alone (the rollout step parses once for its five passes)."""
        # exact float64 positions for the z-matrix step, as the reference (ase.Atoms positions are float64); vectorised, and
        # a `ParsedObservations` (arrays already) is taken as is
        labels, xyz, bags = observation_arrays(observations, self.zs, self.num_atoms)
        pos64, charges, natoms = compact_canvases(labels, xyz, self.zs)
        bags = bags.astype(np.float32)
        return charges, bags, natoms, pos64

    def _placements(self, parsed, actions: np.ndarray):
        """validated action rows (float32) and the two hypothetical placements (dihedral kept / flipped) they imply"""
        charges, bags, natoms, pos64 = parsed
        acts = check_action_rows(actions, len(natoms), 7, 1, 2, self.num_atoms, self.num_zs)
        focus, element = np.rint(acts[:, 1]).astype(np.int64), np.rint(acts[:, 2]).astype(np.int64)
        a64 = acts.astype(np.float64)  # the agent casts actions to its dtype
        new_p = place_new_atoms(pos64, natoms, focus, a64[:, 3], a64[:, 4], a64[:, 5])
        new_m = place_new_atoms(pos64, natoms, focus, a64[:, 3], a64[:, 4], -a64[:, 5])
        z_new = np.asarray(self.zs, dtype=np.int32)[element]
        return acts, new_p, new_m, z_new

    def _cfg(self, natoms) -> _lib.IntCfg:
        """the batch sizes of a step over samples with these atom counts (`gather_totals`: a batch of 2^31 pairs or more raises)"""
        cfg = _lib.IntCfg()
        cfg.B, cfg.N, cfg.Z, cfg.W = len(natoms), self.num_atoms, self.num_zs, self.network_width
        for i, z in enumerate(self.zs):
            cfg.zs[i] = int(z)
        cfg.TA, cfg.MA, cfg.ME = gather_totals(natoms)
        cfg.min_distance, cfg.max_distance = float(self.min_distance), float(self.max_distance)
        return cfg

    _canvas_cfg = _cfg  # (of canvases, from the host mirror of their atom counts: no device round trip)

    def _assemble(self, parsed, placed) -> IntBatch:
        """the ragged 3B-molecule batch (canvas, canvas + new atom at +/- dihedral) of B parsed samples; ONE upload"""
        N = self.num_atoms
        charges, bags, natoms, pos64 = parsed
        acts, new_p, new_m, z_new = placed
        B = len(natoms)
        cfg = self._cfg(natoms)  # (first: the offsets below fit in 32 bits once it has passed)
        TA, MA = cfg.TA, cfg.MA
        real = np.arange(N)[None, :] < natoms[:, None]
        base_z, base_p = charges[real], pos64[real]
        sizes = np.concatenate([natoms, natoms + 1, natoms + 1]).astype(np.int64)
        mol_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        edge_off = np.concatenate([[0], np.cumsum(sizes * (sizes - 1))]).astype(np.int32)
        molZ, molpos = np.zeros(MA, dtype=np.int32), np.zeros((MA, 3))
        molZ[:TA], molpos[:TA] = base_z, base_p
        atom_b = np.repeat(np.arange(B), natoms)
        local = np.arange(TA) - np.repeat(np.cumsum(natoms) - natoms, natoms)
        for s, new in ((1, new_p), (2, new_m)):
            start = mol_off[s * B:(s + 1) * B].astype(np.int64)
            molZ[start[atom_b] + local], molpos[start[atom_b] + local] = base_z, base_p
            molZ[start + natoms], molpos[start + natoms] = z_new, new
        # all six arrays are 4-byte typed: one packed host buffer, one copy, six views
        return IntBatch(cfg, *self._upload_packed(mol_off, edge_off, molZ, molpos.astype(np.float32),
                                                  np.asarray(bags, dtype=np.float32).reshape(B, self.num_zs), acts.reshape(B, 7)))

    def make_batch(self, observations: List[ObservationType], actions: np.ndarray, parsed=None) -> IntBatch:
        if parsed is None:
            parsed = self._parse(observations)
        return self._assemble(parsed, self._placements(parsed, actions))

    def to_action_space(self, action: np.ndarray, observation: ObservationType):
        """(atomic-number index, position) of the atom the 7-column action row places (agent.py:91-110)."""
        stop, focus, element, distance, angle, dihedral, kappa = (float(x) for x in action)
        if stop:
            return None  # the reference builds an empty ase.Atoms here; this agent never stops (agent.py:190-191)
        focus, element = int(round(focus)), int(round(element))
        sign = -1.0 if int(round(kappa)) else 1.0
        atoms = [xyz for label, xyz in observation[0] if self.zs[label] != 0]  # ObservationSpace.parse drops nulls
        n = len(atoms)
        pos = np.zeros((1, max(self.num_atoms, 1), 3))
        for k, xyz in enumerate(atoms):
            pos[0, k] = xyz
        new = place_new_atoms(pos, np.array([n]), np.array([focus]), np.array([distance]), np.array([angle]),
                              np.array([sign * dihedral]))[0]
        index = self.action_space.zs.index(self.observation_space.zs[element])
        return index, tuple(float(x) for x in new)

    def _actions_to_space(self, acts: np.ndarray, pos64: np.ndarray, natoms: np.ndarray, placed=None):
        """to_action_space for a whole batch of action rows: ONE vectorised z-matrix placement instead of one per sample
        (140 single placements are 13 ms of numpy call overhead; this is 0.2 ms) -- same arithmetic, same float64 inputs.
        `placed` = (new_plus, new_minus) of `_placements` for the same rows: the kept / flipped placement is picked, not redone."""
        a64 = np.asarray(acts, dtype=np.float32).astype(np.float64)
        focus, element = np.rint(a64[:, 1]).astype(np.int64), np.rint(a64[:, 2]).astype(np.int64)
        if placed is not None:
            new = np.where((np.rint(a64[:, 6]) != 0)[:, None], placed[1], placed[0])
        else:
            sign = np.where(np.rint(a64[:, 6]) != 0, -1.0, 1.0)
            new = place_new_atoms(pos64, natoms, focus, a64[:, 3], a64[:, 4], sign * a64[:, 5])
        out = []
        for b in range(len(a64)):
            if a64[b, 0]:
                out.append(None)
                continue
            index = self.action_space.zs.index(self.observation_space.zs[int(element[b])])
            out.append((index, tuple(float(x) for x in new[b])))
        return out

    def _forward_nograd(self, batch: IntBatch):
        lib = _lib.lib()
        nbytes = C.c_size_t()
        _lib.check(lib.mg_int_workspace_bytes(C.byref(batch.cfg), C.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.theta.device)
        out = torch.empty(3, batch.cfg.B, dtype=torch.float32, device=self.theta.device)
        with self._guard():
            _lib.check(lib.mg_int_forward(C.byref(batch.cfg), ptr(self.theta), ptr(batch.mol_off),
                                          ptr(batch.edge_off), ptr(batch.molZ), ptr(batch.molpos), ptr(batch.bags),
                                          ptr(batch.actions), ptr(ws), nbytes.value, ptr(out), self._s()))
        self._last_ws = ws
        return out, ws

    def prepare_rollout(self, data: Dict[str, Any]):
        """what `ppo.train` draws its mini-batches from: the rollout a `CarriedRollout` carries (`DeviceRollout.train_data(
        on_device=True)`), unchanged; host data parked in HBM when `gather_on_device` is set; `IntRollout` otherwise"""
        if isinstance(data['obs'], CarriedRollout):
            return data['obs'].rollout
        if self.gather_on_device:
            return IntRolloutOnDevice.from_host(self, data)
        return IntRollout(self, data)

    def prepare_batch(self, observations, actions, logp=None, adv=None, ret=None) -> IntBatch:
        batch = self.make_batch(observations, actions)
        batch.logp, batch.adv, batch.ret = self._f64(logp), self._f64(adv), self._f64(ret)
        return batch

    # ---- what depends on theta alone, once per EPOCH (ppo.py:117-146: one optimizer step per epoch), as CovariantAC does ----
    def invalidate_weights(self) -> None:
        """theta may have changed (start of a PPO epoch): the derived weight matrices cached in the workspaces are stale"""
        for st in self._ws_epoch.values():
            st['weights'] = False

    def fold_gradients(self) -> None:
        """(interface of ppo.train's epoch loop: this agent has no expanded weight gradients to fold -- theta.grad is complete
        after every mini-batch)"""

    def _step_workspace(self, cfg, slot: int) -> torch.Tensor:
        """one cached block per slot (the derived weights sit first in it, at offsets that do not depend on the batch)"""
        nbytes = C.c_size_t()
        _lib.check(_lib.lib().mg_int_workspace_bytes(C.byref(cfg), C.byref(nbytes)))
        ws, replaced = self._cached_block(slot, nbytes.value)
        if replaced:
            self._ws_epoch.pop(slot, None)
        ws.record_stream(torch.cuda.current_stream(self.theta.device))
        return ws

    def ppo_minibatch(self, batch: IntBatch, clip_ratio: float, vf_coef: float, entropy_coef: float,
                      loss_scale: float = 1.0, slot: int = 0, stats_accum: Optional[torch.Tensor] = None,
                      graph: Optional[bool] = None, epoch_cache: bool = False,
                      grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """forward + float64 PPO loss + hand-written backward on the device (ppo.py:124-131) in ONE C call (mg_int_ppo_step),
        gradients accumulated into theta.grad (scaled by `loss_scale`: the data-parallel B_local / B_global); same signature
        and meaning as CovariantAC.ppo_minibatch: `stats_accum` receives loss_scale x statistics on the device, `graph` (default
        on) issues the launches as one hipGraph launch whose kernel nodes are updated in place, one cached graph per `slot`;
        `epoch_cache` (ppo.train's loop): the derived weight matrices of this slot's workspace are prepared by the slot's FIRST
        mini-batch after `invalidate_weights()` only.  `grad_out` (flat float32, theta's size; default theta.grad) receives the
        gradient instead: ppo.train's ordered data-parallel mode keeps one row per mini-batch.  Returns the 6 loss statistics
        (float64 device tensor, no sync)."""
        ws = self._step_workspace(batch.cfg, slot)
        flags = 0
        if epoch_cache:
            st = self._ws_epoch.setdefault(slot, {'weights': False})
            flags = _lib.STEP_WEIGHTS_CURRENT if st['weights'] else 0
            st['weights'] = True
        else:
            self._ws_epoch.pop(slot, None)

        def call(out, gout, stats, grad, graph_slot, used):
            _lib.check(_lib.lib().mg_int_ppo_step(C.byref(batch.cfg), ptr(self.theta), ptr(batch.mol_off), ptr(batch.edge_off),
                                                  ptr(batch.molZ), ptr(batch.molpos), ptr(batch.bags), ptr(batch.actions), ptr(ws),
                                                  ws.numel(), ptr(batch.logp), ptr(batch.adv), ptr(batch.ret), clip_ratio, vf_coef,
                                                  entropy_coef, float(loss_scale), ptr(out), ptr(gout), ptr(stats), ptr(stats_accum),
                                                  ptr(grad), graph_slot, flags, used, self._s()))

        return self._ppo_frame(batch, ws, slot, graph, grad_out, call)

    def _ws_view(self, cfg, ws: torch.Tensor, name: str) -> torch.Tensor:
        off, cnt = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().mg_int_workspace_lookup(C.byref(cfg), name.encode(), C.byref(off), C.byref(cnt)))
        return ws.view(torch.float32)[off.value:off.value + cnt.value]

    def _step_sample(self, observations: List[ObservationType]) -> Dict[str, Any]:
        """step(obs) of the rollout (agent.py:181-353 with actions=None).  The sub-actions are conditioned on each
        other (element on the focus, the continuous means on both, kappa on the placed atom), so the evaluation
        kernels run once per stage on the partially filled action rows; every draw uses torch's device RNG
        (Categorical / Normal as in the reference, so torch.manual_seed governs rollouts), argmax / means in
        evaluation mode.  The last pass is the plain evaluation of the completed rows, so logp / ent / v are
        exactly what step(obs, actions) returns for them."""
        B, N, Z = len(observations), self.num_atoms, self.num_zs
        dev = self.theta.device
        parsed = self._parse(observations)
        _, bags, natoms, pos64 = parsed
        acts = np.zeros((B, 7), dtype=np.float32)  # stop = 0: this agent does not stop
        acts[:, 3] = 0.5 * (self.min_distance + self.max_distance)  # harmless placeholders for the early passes
        acts[:, 4] = acts[:, 5] = 0.5 * np.pi
        nat = torch.from_numpy(natoms.astype(np.int64)).to(dev)
        with torch.no_grad():
            # [r5] focus, element and the three continuous sub-actions only read the BASE molecules' latents (the +/- dihedral
            # copies feed the kappa head alone), so their three passes share ONE assembled batch whose action rows are completed on
            # the device as the draws are made; the placements are computed once all of them are known: two assemblies and uploads
            # and one device -> host copy where there were five and four
            # focus (agent.py:206-221): softmax over the real atoms; an empty canvas focuses slot 0
            # (the first assembly's +/- copies get their new atom far outside every cutoff: nothing reads their latents yet)
            far = 1.0e3 + 10.0 * np.arange(B, dtype=np.float64)[:, None] * np.ones((1, 3))
            batch = self._assemble(parsed, (acts, far, far, np.full(B, self.zs[0], dtype=np.int32)))
            _, ws = self._forward_nograd(batch)
            logit_f = self._ws_view(batch.cfg, ws, 'logitF')[:batch.cfg.TA]
            dense = torch.full((B, N), float('-inf'), device=dev)
            slot = torch.arange(N, device=dev)[None, :] < nat[:, None]
            dense[slot] = logit_f
            dense[nat == 0, 0] = 0.0
            p_f = torch.softmax(dense, dim=-1)
            # (torch.multinomial / torch.normal directly: what Categorical.sample / Normal.sample call, same draws from the same RNG stream)
            focus = torch.multinomial(p_f / p_f.sum(-1, keepdim=True), 1, True).squeeze(1) if self.training else torch.argmax(p_f, -1)
            batch.actions[:, 1] = focus.to(torch.float32)
            # element (agent.py:229-242): softmax over the elements left in the bag
            _, ws = self._forward_nograd(batch)
            logit_e = self._ws_view(batch.cfg, ws, 'logitE')[:B * Z].view(B, Z)
            mask_e = torch.from_numpy(bags > 0).to(dev)
            dense = torch.where(mask_e, logit_e, torch.full_like(logit_e, float('-inf')))
            dense[~mask_e.any(dim=-1), 0] = 0.0  # an exhausted bag never reaches the agent; keep the draw defined
            p_e = torch.softmax(dense, dim=-1)
            element = torch.multinomial(p_e / p_e.sum(-1, keepdim=True), 1, True).squeeze(1) if self.training else torch.argmax(p_e, -1)
            batch.actions[:, 2] = element.to(torch.float32)
            # distance / angle / dihedral (agent.py:246-292): Normal around tanh(mean) * width / 2 + center
            _, ws = self._forward_nograd(batch)
            cout = self._ws_view(batch.cfg, ws, 'cout')[:B * 3].view(B, 3)
            half_w = torch.tensor([0.5 * (self.max_distance - self.min_distance), 0.5 * np.pi, 0.5 * np.pi], device=dev)
            center = torch.tensor([0.5 * (self.max_distance + self.min_distance), 0.5 * np.pi, 0.5 * np.pi], device=dev)
            mean = torch.tanh(cout) * half_w + center
            if self.training:
                o, shp = self.slot_table['log_stds']
                scale = torch.exp(1e-6 + self.theta[o:o + 3])
                cont = torch.normal(mean, scale.expand_as(mean))
                cont[:, 0].clamp_(min=0.001)  # the sampled distance must stay positive (agent.py:254-255)
            else:
                cont = mean
            drawn = torch.cat([focus.to(torch.float32)[:, None], element.to(torch.float32)[:, None], cont.to(torch.float32)], dim=1)
            acts[:, 1:6] = drawn.cpu().numpy()
            # kappa (agent.py:294-315): keep / flip the dihedral, logits from the two hypothetical placements
            placed = self._placements(parsed, acts)
            batch = self._assemble(parsed, placed)
            _, ws = self._forward_nograd(batch)
            kv = self._ws_view(batch.cfg, ws, 'kv')[:2 * B].view(2, B).t()
            kappa = torch.multinomial(torch.softmax(kv, dim=-1), 1, True).squeeze(1) if self.training else torch.argmax(kv, -1)
            batch.actions[:, 6] = kappa.to(torch.float32)
            out, _ = self._forward_nograd(batch)  # the plain evaluation of the completed rows
            acts[:, 6] = kappa.cpu().numpy()
        return {'a': batch.actions, 'logp': out[0], 'ent': out[1], 'v': out[2],
                'actions': self._actions_to_space(acts, pos64, natoms, placed[1:3])}

    def step(self, observations: List[ObservationType], actions: Optional[np.ndarray] = None) -> Dict[str, Any]:
        self._require_device()
        if actions is None:
            return self._step_sample(observations)
        parsed = self._parse(observations)
        batch = self.make_batch(observations, actions, parsed)
        out = _IntStep.apply(self.theta, self, batch)
        acts = np.asarray(actions, dtype=np.float32)
        return {'a': batch.actions, 'logp': out[0], 'ent': out[1], 'v': out[2],
                'actions': self._actions_to_space(acts, parsed[3], parsed[2])}

    # -- persistent device canvases (`make_canvas`): the whole sampling step on the device, one C call ----------------------------
    def _draw_par(self):
        """half widths and centres of distance / angle / dihedral as float32, computed as `_step_sample` computes them"""
        if self._draw_par_c is None:
            half_w = [0.5 * (self.max_distance - self.min_distance), 0.5 * np.pi, 0.5 * np.pi]
            center = [0.5 * (self.max_distance + self.min_distance), 0.5 * np.pi, 0.5 * np.pi]
            self._draw_par_c = (C.c_float * 6)(*np.asarray(half_w + center, dtype=np.float32).tolist())
        return self._draw_par_c

    def _sample_workspace(self, cfg) -> torch.Tensor:
        nbytes = C.c_size_t()
        _lib.check(_lib.lib().mg_int_sample_workspace_bytes(C.byref(cfg), C.byref(nbytes)))
        return self._cached_block('sample', nbytes.value)[0]

    def _sample_canvas(self, canvas, seed: Optional[int], sample_ids: Tuple[int, int], acts: torch.Tensor, newpos: torch.Tensor,
                       out: torch.Tensor, err: torch.Tensor):
        """the sampling launch of `step_canvas` alone (also `episodes.DeviceEpisodes.step`): ONE C call draws the action rows
        `acts` (E, 7), places them (`newpos` (E, 3) float64) and evaluates logp / ent / v `out` (3, E); `err` (int32) is the
        flag of canvases that disagree with the host mirror of the atom counts.  Nothing is copied to the host."""
        self._require_device()
        cfg = self._cfg(canvas.natoms)
        ws = self._sample_workspace(cfg)
        if seed is None:
            seed = self.draw_seed()
        mode = 1 if self.training else 2
        with self._guard():
            _lib.check(_lib.lib().mg_int_sample_ids(C.byref(cfg), ptr(self.theta), ptr(canvas.pos64), ptr(canvas.pos32),
                                                    ptr(canvas.charges), ptr(canvas.bags), ptr(canvas.natoms_dev), C.c_uint64(seed),
                                                    int(sample_ids[0]), int(sample_ids[1]), mode, self._draw_par(), ptr(ws),
                                                    ws.numel(), ptr(acts), ptr(newpos), ptr(out), ptr(err), self._s()))
        self._last_ws, self._last_sample_cfg = ws, cfg
        return cfg

    def step_canvas(self, canvas, commit: bool = True, seed: Optional[int] = None,
                    sample_ids: Tuple[int, int] = (0, 1)) -> Dict[str, Any]:
        """step(observations) of the rollout on resident canvases (`make_canvas`): the same return dict, drawn by ONE C call
        (mg_int_sample_ids: batch assembly, the five passes, the draws and the float64 z-matrix placement on the device) and
        read back by ONE device-to-host copy (action rows, placed positions, error flag).  With `commit` the drawn atoms are
        then placed on the canvases in HBM.  `seed` / `sample_ids = (base, stride)`: row b draws from the random stream
        (seed, base + stride * b), as `CovariantAC.step_canvas`.  Training mode draws, evaluation takes argmax / means."""
        self._require_device()
        B = canvas.E
        natoms_before = canvas.natoms.copy()
        dev = self.theta.device
        # one buffer for everything the host reads: [newpos f64 (B, 3) | action rows f32 (B, 7) | error flag i32]
        o_act, o_err = 24 * B, 24 * B + 28 * B
        res = torch.empty(o_err + 8, dtype=torch.uint8, device=dev)
        newpos = res[:o_act].view(torch.float64).view(B, 3)
        acts = res[o_act:o_err].view(torch.float32).view(B, 7)
        out = torch.empty(3, B, dtype=torch.float32, device=dev)
        self._sample_canvas(canvas, seed, sample_ids, acts, newpos, out, res[o_err:])
        host = res.cpu().numpy()
        err = int(host[o_err:o_err + 4].view(np.int32)[0])
        if err:
            raise RuntimeError(f'molgym_hip error -1: the device canvases disagree with the host mirror of the atom counts '
                               f'(flag {err}); nothing was drawn or placed')
        canvas.place(acts, newpos, commit)
        host_p = host[:o_act].view(np.float64).reshape(B, 3)
        host_a = host[o_act:o_err].view(np.float32).reshape(B, 7)
        elements = np.rint(host_a[:, 2]).astype(np.int64)
        if commit:
            canvas.commit_mirror(natoms_before, elements, host_p)
        index = [self.action_space.zs.index(z) for z in self.observation_space.zs]
        actions = [(index[int(e)], (float(q[0]), float(q[1]), float(q[2]))) for e, q in zip(elements, host_p)]
        return {'a': acts, 'logp': out[0], 'ent': out[1], 'v': out[2], 'actions': actions}
