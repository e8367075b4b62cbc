"""Covariant (Cormorant) actor-critic on the gfx950 HIP kernels.

Drop-in for /root/reference/molgym/agents/covariant/agent.py:20-334: same
constructor keywords (model_util.py:26-39), same ``step(observations, actions)``
contract (base.py:17-19).  All arithmetic of ``step`` with actions given -- the PPO
training path, ppo.py:26 -- runs in libmolgym_hip.so through one autograd node;
there is no eager / CPU fallback.
"""
import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib, layout
from ..lebedev import lebedev_table
from ..observations import CarriedRollout, compact_canvases, observation_arrays, parse_observations_host  # noqa: F401 (re-exported)
from ..spaces import ActionSpace, ObservationSpace, ObservationType
from .base import FlatThetaAgent, check_action_rows
from .dists import StepDists

ptr = _ptr = _lib.ptr  # (`_ptr`, `_stream`: the names this module had for them)


def _stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class DeviceBatch:
    """One PPO mini-batch resident in HBM (layout of include/molgym_hip.h)."""

    def __init__(self, cfg, pos, charges, bags, actions, logp=None, adv=None, ret=None):
        self.cfg, self.pos, self.charges, self.bags, self.actions = cfg, pos, charges, bags, actions
        self.logp, self.adv, self.ret = logp, adv, ret


class RolloutOnDevice:
    """A parsed rollout resident in HBM; `minibatch(indices)` gathers one PPO mini-batch on the device."""

    def __init__(self, ac, natoms, pos, charges, bags, actions, logp, adv, ret):
        self.ac, self.natoms = ac, natoms
        self.t = (pos, charges, bags, actions, logp, adv, ret)

    def minibatch(self, indices: np.ndarray, idx_dev: Optional[torch.Tensor] = None) -> DeviceBatch:
        """`idx_dev`: the same indices already on the device (ppo.train uploads an epoch's permutation once)"""
        if idx_dev is None:
            idx_dev = torch.as_tensor(np.asarray(indices, dtype=np.int64)).to(self.t[0].device)
        with self.ac._guard():
            pos, charges, bags, actions, logp, adv, ret = _lib.gather_rows(self.t, idx_dev, self.ac._s())
        return DeviceBatch(self.ac._make_cfg(len(indices), self.natoms[indices]), pos, charges, bags, actions, logp,
                           adv, ret)


def _refuse_deterministic(what: str) -> None:
    """deterministic mode (molgym_amd.set_deterministic) by itself orders SchNetAC's gradient sums only: this agent's default
    kernels accumulate with float atomics, and refusing beats being silently non-deterministic.  Its own ordered mode is a second
    opt-in (`covariant=True`): it gives up the fused small-batch kernels and the graph launch and costs scratch per edge."""
    if _lib.is_deterministic() and not _lib.is_deterministic_covariant():
        raise RuntimeError(f'CovariantAC.{what}: deterministic mode covers SchNetAC only '
                           '(molgym_amd.set_deterministic(False) to train this agent, or '
                           'molgym_amd.set_deterministic(True, covariant=True) for its ordered, slower path)')


class _CovStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, ac, cfg, pos, charges, bags, actions):
        lib = ac._L()
        nbytes = C.c_size_t()
        _lib.check(lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(nbytes)), lib)
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=theta.device)
        out = torch.empty(3, cfg.B, dtype=torch.float32, device=theta.device)
        with torch.cuda.device(theta.device):
            _lib.check(lib.mg_cov_forward(C.byref(cfg), ptr(theta), ptr(pos), ptr(charges), ptr(bags),
                                          ptr(actions), ptr(ac.leb), ptr(ws), nbytes.value, ptr(out),
                                          ac._s()), lib)
        ctx.save_for_backward(theta, pos, charges, bags, actions, ws)
        ctx.cfg, ctx.ac = cfg, ac
        ac._last_ws = ws
        return out

    @staticmethod
    def backward(ctx, gout):
        _refuse_deterministic('step(...).backward()')
        theta, pos, charges, bags, actions, ws = ctx.saved_tensors
        lib = ctx.ac._L()
        grad = torch.zeros_like(theta)
        gout = gout.contiguous()
        with torch.cuda.device(theta.device):
            _lib.check(lib.mg_cov_backward(C.byref(ctx.cfg), ptr(theta), ptr(pos), ptr(charges), ptr(bags),
                                           ptr(actions), ptr(ctx.ac.leb), ptr(ws), ws.numel(), ptr(gout),
                                           ptr(grad), ctx.ac._s()), lib)
        return grad, None, None, None, None, None, None


class CovariantAC(FlatThetaAgent):
    action_cols = 6  # (focus, element, distance, x, y, z)
    # `_unchecked`: per slot, the (cfg, workspace) of a launch whose list-build flags nobody has read yet; `_grad_k`, `_iota`:
    # the kernel-side gradient buffers and the index of their gather at maxl < 4
    _TRANSIENT = FlatThetaAgent._TRANSIENT + (('_unchecked', dict), ('_grad_k', dict), ('_iota', None))

    def __init__(
        self,
        observation_space: ObservationSpace,
        action_space: ActionSpace,
        min_max_distance: Tuple[float, float],
        network_width: int,
        maxl: int,
        num_cg_levels: int,
        num_channels_hidden: int,
        num_channels_per_element: int,
        num_gaussians: int,
        bag_scale: int,
        beta: Optional[float] = None,
        device=None,
    ):
        super().__init__(observation_space, action_space)
        canvas_size = self.observation_space.canvas_space.size
        if not 1 <= canvas_size <= _lib.MG_MAX_CANVAS:
            # (<= 64 atoms: all heads in one launch per direction; larger canvases: the staged head kernels)
            raise RuntimeError(f'canvas_size {canvas_size}: the HIP kernels support canvases of 1..{_lib.MG_MAX_CANVAS} atoms')
        num_zs = len(self.observation_space.zs)
        if not 2 <= num_zs <= _lib.MG_MAX_Z:
            raise RuntimeError(f'len(zs) {num_zs}: the HIP kernels support element sets of 2..{_lib.MG_MAX_Z} symbols')
        if num_zs * int(num_channels_per_element) > _lib.MG_MAX_ZCE:
            # (the last atom level mixes into 2 * len(zs) * num_channels_per_element real columns; the GEMM forms stop at 128)
            raise RuntimeError(f'len(zs) {num_zs} x num_channels_per_element {num_channels_per_element} = '
                               f'{num_zs * int(num_channels_per_element)}: the HIP kernels support a product of up to '
                               f'{_lib.MG_MAX_ZCE} ({_lib.MG_MAX_ZCE // int(num_channels_per_element)} symbols at this channel count)')
        if not 1 <= int(maxl) <= layout.MAXL:
            raise RuntimeError(f'maxl {maxl}: the gfx950 kernels cover 1..{layout.MAXL} (the Clebsch-Gordan tables, thread maps and LDS '
                               f'layouts are laid out for the 25 (l, m) rows of maxl = 4, the reference default, arg_parser.py:56; a '
                               f'smaller maxl runs as the same network with the higher degrees structurally zero)')
        if not _lib.LEVELS_RANGE[0] <= int(num_cg_levels) <= _lib.LEVELS_RANGE[1]:
            raise RuntimeError(f'num_cg_levels {num_cg_levels}: the kernels cover {_lib.LEVELS_RANGE[0]}..{_lib.LEVELS_RANGE[1]}')
        # the channel counts and num_cg_levels are compile-time constants of a library build: the defaults load
        # libmolgym_hip.so, other values their own build of the same sources (compiled on first use,
        # molgym_amd/_lib.py::build_variant)
        self._channels = (int(num_channels_hidden), int(num_channels_per_element), int(num_cg_levels))
        self.device = torch.device(device) if device is not None else torch.device('cuda')
        self.dtype = torch.float
        self.zs = list(self.observation_space.zs)
        self.min_distance, self.max_distance = min_max_distance
        assert self.min_distance < self.max_distance
        self.beta = beta
        self.max_sh, self.num_cg_levels = maxl, num_cg_levels
        self.num_channels_hidden, self.num_channels_per_element = num_channels_hidden, num_channels_per_element
        if network_width > 1024 or network_width % 4:
            # (<= 128: all heads in one launch per direction; wider: the staged head kernels + row GEMMs, any multiple of 4)
            raise RuntimeError(f'network_width {network_width}: the HIP heads kernels support multiples of 4 up to 1024')
        self.num_gaussians, self.network_width, self.bag_scale = num_gaussians, network_width, bag_scale
        self.num_channels_out = len(self.zs) * num_channels_per_element
        self.slot_table, total = layout.offsets(len(self.zs), network_width, num_gaussians, *self._channels, int(maxl))  # (C, Ce, levels, maxl)
        self._L()  # load (build) the library for these channel counts now: a missing toolchain fails here, not mid-rollout
        self.theta = torch.nn.Parameter(self._init_theta(total))
        self.register_buffer('leb', torch.from_numpy(lebedev_table()), persistent=False)
        # [r6] maxl < 4 (arg_parser.py:56): theta / state_dict are the maxl-limited module's (the reference's shapes); the kernels
        # read the maxl = 4 layout, into which theta is EMBEDDED -- the smaller network is the larger one with every quantity of a
        # degree above maxl multiplied by a zero weight, so outputs are those of the smaller network and its gradient is the gather
        # of the larger one's (layout.embedding_index; exact: tests/test_host.py checks it on the oracle, the GPU tests against the
        # oracle built with the same maxl).  Not faster than maxl = 4: the kernels still walk the 25 (l, m) rows.
        if int(maxl) < layout.MAXL:
            _, total_k = layout.offsets(len(self.zs), network_width, num_gaussians, *self._channels)
            idx = layout.embedding_index(len(self.zs), network_width, num_gaussians, *self._channels, int(maxl))
            self.register_buffer('_embed_idx', torch.from_numpy(idx), persistent=False)
            self.register_buffer('_theta_k', torch.zeros(total_k), persistent=False)
        self.to(self.device)

    def _chk(self, rc):
        _lib.check(rc, self._L())

    def _L(self):
        """the library build for this agent's channel counts"""
        return _lib.lib(getattr(self, '_channels', None))

    # -- the parameter vector the KERNELS read (maxl = 4 layout) and the gradient buffer they add into ----------------------
    def _ktheta(self, refresh: bool = True) -> torch.Tensor:
        if self.max_sh == layout.MAXL:
            return self.theta
        if refresh:  # (positions outside the index are zero from construction and never written; rewriting equal values is
            with torch.no_grad():  # harmless to a kernel of another stream that reads them meanwhile)
                self._theta_k.index_copy_(0, self._embed_idx, self.theta.detach())
        return self._theta_k

    def _kgrad(self, slot: int = 0, grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.max_sh == layout.MAXL:
            return self.theta.grad if grad_out is None else grad_out
        bufs = self._grad_k
        if slot not in bufs or bufs[slot].device != self.theta.device:
            bufs[slot] = torch.zeros_like(self._theta_k)
        return bufs[slot]

    def _kgrad_collect(self, slot: int, grad_out: Optional[torch.Tensor] = None) -> None:
        """maxl < 4: theta.grad (or `grad_out`) += gather of the slot's kernel-side gradient buffer (float atomics: mini-batches
        of other streams may be adding to theta.grad too), buffer zeroed for its next use"""
        if self.max_sh == layout.MAXL:
            return
        gk = self._grad_k[slot]
        if self._iota is None or self._iota.device != self.theta.device:
            self._iota = torch.arange(self.theta.numel(), device=self.theta.device)
        (self.theta.grad if grad_out is None else grad_out).index_add_(0, self._iota, gk.index_select(0, self._embed_idx))
        gk.zero_()

    # -- parameters -----------------------------------------------------------------------------
    def _init_theta(self, total: int) -> torch.Tensor:
        """Same initialisers as the reference stack: torch Linear defaults for the radial / input
        Linear layers, U(-1,1)*gain/max(dims) for the complex mixes ('rand'), orthogonal + zero bias
        for the MLPs (modules.py:30-34), log 0.1 for the GMM widths (agent.py:134-136)."""
        theta = torch.zeros(total)
        for name, (off, shape) in self.slot_table.items():
            n = int(np.prod(shape))
            view = theta[off:off + n].view(shape)
            if name.endswith('scales'):
                view.copy_(torch.tensor([0., 1., 2., 3., 0., 1., 2., 3.]).view(shape))
            elif name.endswith('phases'):
                view.copy_(torch.tensor([0.] * 4 + [np.pi / 2] * 4).view(shape))
            elif 'cat_mix.weights' in name:
                gain = 1.0 if 'edge_levels' in name else 10.0
                view.copy_((2 * torch.rand(shape) - 1) * (gain / max(shape)))
            elif name.startswith('phi_') and name.endswith('weight'):
                torch.nn.init.orthogonal_(view)
            elif name.startswith('phi_') and name.endswith('bias'):
                view.zero_()
            elif name == 'distance_log_stds':
                view.fill_(float(np.log(0.1)))
            elif ('.linear.' in name or name.endswith('lin.weight')) and name.endswith('weight'):
                lin = torch.nn.Linear(shape[1], shape[0])
                view.copy_(lin.weight.data)
                self._pending_bias = lin.bias.data.clone()
            elif name.endswith('bias'):
                view.copy_(self._pending_bias)
            else:
                raise RuntimeError(f'no initialiser for {name}')
        if hasattr(self, '_pending_bias'):
            del self._pending_bias
        return theta

    # -- batch ----------------------------------------------------------------------------------
    def _make_cfg(self, B: int, natoms: np.ndarray) -> _lib.CovCfg:
        cfg = _lib.CovCfg()
        cfg.B, cfg.N, cfg.Z = B, self.observation_space.canvas_space.size, len(self.zs)
        for i, z in enumerate(self.zs):
            cfg.zs[i] = int(z)
        cfg.W, cfg.G = self.network_width, self.num_gaussians
        cfg.TA, cfg.TE = int(natoms.sum()), int((natoms.astype(np.int64)**2).sum())
        cfg.has_beta = 0 if self.beta is None else 1
        cfg.beta = 0.0 if self.beta is None else float(self.beta)
        cfg.bag_scale = float(self.bag_scale)
        cfg.min_distance, cfg.max_distance = float(self.min_distance), float(self.max_distance)
        return cfg

    def to_action_space(self, action: np.ndarray, observation: ObservationType):
        """agent.py:147-163 without the ase round trip: position = focused atom + distance * direction, where the
        focus indexes the non-null canvas items in canvas order (ObservationSpace.parse drops the null items,
        spaces.py:55-61,106-107)."""
        assert action.shape == (6, )
        focus, element_index = int(round(float(action[0]))), int(round(float(action[1])))
        atoms = [xyz for label, xyz in observation[0] if self.zs[label] != 0]
        if len(atoms):
            position = tuple(np.asarray(atoms[focus], dtype=np.float64) + action[2] * action[3:6])
        else:
            position = (0.0, 0.0, 0.0)
        return element_index, position

    def _check_actions(self, actions, B: int) -> np.ndarray:
        return check_action_rows(actions, B, 6, 0, 1, self.observation_space.canvas_space.size, len(self.zs))

    def _dists(self, cfg, ws: torch.Tensor, bags: torch.Tensor) -> StepDists:
        block = torch.empty(StepDists.block_floats(cfg), dtype=torch.float32, device=self.theta.device)
        with self._guard():
            self._chk(self._L().mg_cov_head_outputs(C.byref(cfg), ptr(ws), ws.numel(), ptr(block), self._s()))
        return StepDists(self, cfg, block, bags)

    def step(self, observations: List[ObservationType], actions: Optional[np.ndarray] = None) -> Dict[str, Any]:
        self._require_device()
        if actions is None:
            return self._step_sample(observations)
        N = self.observation_space.canvas_space.size
        pos, charges, bags, natoms = parse_observations_host(observations, self.zs, N)
        B = len(observations)
        acts = self._check_actions(actions, B)
        cfg = self._make_cfg(B, natoms)
        d_pos, d_chg, d_bag, d_act = self._upload_packed(pos, charges, bags, acts)
        theta = self.theta
        if self.max_sh != layout.MAXL:  # (differentiable embedding: autograd gathers the gradient back)
            theta = torch.zeros_like(self._theta_k).index_copy(0, self._embed_idx, self.theta)
        out = _CovStep.apply(theta, self, cfg, d_pos, d_chg, d_bag, d_act)
        return {'a': d_act, 'logp': out[0], 'ent': out[1], 'v': out[2],
                'dists': self._dists(cfg, self._last_ws, d_bag)}

    # -- device-resident mini-batches (the PPO fast path: no autograd graph, no host sync) ---------
    def prepare_batch(self, observations: List[ObservationType], actions: np.ndarray, logp=None, adv=None,
                      ret=None) -> 'DeviceBatch':
        """Parse on the host once and park everything a PPO mini-batch needs in HBM."""
        N = self.observation_space.canvas_space.size
        pos, charges, bags, natoms = parse_observations_host(observations, self.zs, N)
        B = len(observations)
        acts = self._check_actions(actions, B)
        d_pos, d_chg, d_bag, d_act = self._upload_packed(pos, charges, bags, acts)
        return DeviceBatch(self._make_cfg(B, natoms), d_pos, d_chg, d_bag, d_act, self._f64(logp), self._f64(adv), self._f64(ret))

    def prepare_rollout(self, data: Dict[str, Any]) -> 'RolloutOnDevice':
        """Parse a whole rollout (the `data` dict of ppo.train) once; mini-batches are device gathers.  A rollout recorded on
        the device (`DeviceRollout.train_data()`) carries its prepared form and is handed back unchanged."""
        if isinstance(data['obs'], CarriedRollout):
            return data['obs'].rollout
        N = self.observation_space.canvas_space.size
        pos, charges, bags, natoms = parse_observations_host(data['obs'], self.zs, N)
        acts = self._check_actions(data['act'], len(data['obs']))
        d_pos, d_chg, d_bag, d_act = self._upload_packed(pos, charges, bags, acts)
        return RolloutOnDevice(self, natoms, d_pos, d_chg, d_bag, d_act, *(self._f64(data[k]) for k in ('logp', 'adv', 'ret')))

    def _workspace(self, cfg: _lib.CovCfg, slot: int = 0, epoch_step: bool = False) -> torch.Tensor:
        nbytes = C.c_size_t()
        self._chk(self._L().mg_cov_workspace_bytes(C.byref(cfg), C.byref(nbytes)))
        st, old = self._ws_epoch.get(slot), self._ws_cache.get(slot)
        ws, replaced = self._cached_block(slot, nbytes.value)
        # Only THIS slot is folded here, on the current stream = the stream this slot's mini-batches were issued on
        # (ppo._DeviceRunner.run): the other slots' backward launches may still be adding to their accumulators on their own
        # streams, and k_fold_weights reads-then-zeroes non-atomically -- folding them from here would lose what lands in between.
        # Folded is the block that holds an epoch's deferred weight gradients: before another kind of call uses it, or as it
        # is replaced.
        if st is not None and st.get('pending') and (replaced or not epoch_step):
            self._fold_slot(slot, st, old)
        if replaced:
            self._ws_epoch.pop(slot, None)
        # the cached block may have been allocated under another stream (rollout: default stream; ppo.train: its own): tell
        # the caching allocator about THIS use, so that a later replacement is not handed out while kernels still read it
        ws.record_stream(torch.cuda.current_stream(self.theta.device))
        return ws

    # ---- what depends on theta alone, once per EPOCH instead of once per mini-batch (ppo.py:117-146: one optimizer step per epoch) ----
    def invalidate_weights(self) -> None:
        """theta may have changed (start of a PPO epoch): the derived weight matrices cached in the workspaces are stale"""
        self._ktheta()  # (maxl < 4: re-embed theta, on the caller's stream -- ppo._DeviceRunner.begin_epoch orders the others behind it)
        for st in self._ws_epoch.values():
            st['weights'] = False
            # A slot still pending HERE was left by an epoch that never reached its fold (an exception between its mini-batches
            # and end_epoch): what its accumulator holds belongs to a gradient that was abandoned.  Drop the claim -- the slot's
            # next epoch_cache step prepares the weights anew, which zeroes the accumulator; a slot the new epoch never touches is
            # then NOT folded into the new theta.grad by end_epoch.
            st['pending'] = False

    def fold_gradients(self, slot: Optional[int] = None) -> None:
        """mg_cov_fold_grads for every workspace (`slot=None`) -- or the one of `slot` -- whose mini-batches ran with
        `epoch_cache=True` since the last fold: theta.grad is complete only after the all-slot call (ppo.train: once per epoch,
        before the all-reduce / norm / clip / Adam step).  Issued on the current stream, which must already be ordered behind
        the streams of the slots it folds (all of them: ppo._DeviceRunner.end_epoch after its wait_stream joins; one: the
        slot's own stream, _workspace)."""
        for sl, st in self._ws_epoch.items():
            if (slot is None or sl == slot) and st.get('pending'):
                self._fold_slot(sl, st, self._ws_cache[sl])

    def _fold_slot(self, slot: int, st: dict, ws: torch.Tensor) -> None:
        with self._guard():
            self._chk(self._L().mg_cov_fold_grads(C.byref(st['cfg']), ptr(ws), ws.numel(), ptr(self._kgrad(slot)), self._s()))
        self._kgrad_collect(slot)
        ws.record_stream(torch.cuda.current_stream(self.theta.device))
        st['pending'] = False

    def forward_batch(self, batch: 'DeviceBatch', slot: int = 0) -> torch.Tensor:
        """(3, B) float32: logp, ent, v -- no autograd graph."""
        ws = self._workspace(batch.cfg, slot)
        out = torch.empty(3, batch.cfg.B, dtype=torch.float32, device=self.theta.device)
        with self._guard():
            self._chk(self._L().mg_cov_forward(C.byref(batch.cfg), ptr(self._ktheta()), ptr(batch.pos),
                                                 ptr(batch.charges), ptr(batch.bags), ptr(batch.actions),
                                                 ptr(self.leb), ptr(ws), ws.numel(), ptr(out), self._s()))
        self._last_ws, self._last_cfg = ws, batch.cfg
        # every (cfg, workspace) a training forward used since the last check: ppo.train keeps three mini-batches in flight on
        # their own workspaces, and the list build raises its error flags in the workspace of the mini-batch it belongs to
        self._unchecked[slot] = (batch.cfg, ws)
        return out

    def check_inputs(self) -> None:
        """Surface the list-build flags of EVERY training forward since the last call (mg_cov_check: canvases whose atoms are
        not compacted to the front, TA / TE that do not match the charges) as RuntimeError -- one (cfg, workspace) pair per
        workspace slot, i.e. the most recent mini-batch of each stream ppo.train keeps in flight.  It reads 16 bytes back per
        slot, i.e. synchronises: ppo.train calls it once per call, right after the first epoch's own device -> host copy.
        A rank that evaluated nothing since the last call checks nothing (no stale cfg against a workspace the rollout's
        sampling launches have since reused)."""
        pending, self._unchecked = self._unchecked, {}
        with self._guard():
            for cfg, ws in pending.values():
                self._chk(self._L().mg_cov_check(C.byref(cfg), ptr(ws), ws.numel(), self._s()))

    def input_flags_async(self) -> Optional[torch.Tensor]:
        """the list-build flags check_inputs() would read, as ONE pinned host tensor filled by asynchronous copies on the current
        stream (one int per workspace slot used since the last check; None if there is nothing to check): the caller waits for
        an event it records behind this call and hands the tensor to `raise_input_flags` -- ppo.train's run-ahead loop never
        drains the stream for the check."""
        pending, self._unchecked = list(self._unchecked.values()), {}
        if not pending:
            return None
        host = torch.empty(len(pending), dtype=torch.int32).pin_memory()
        for k, (cfg, ws) in enumerate(pending):
            off, cnt = C.c_int64(), C.c_int64()
            self._chk(self._L().mg_cov_workspace_lookup(C.byref(cfg), b'err', C.byref(off), C.byref(cnt)))
            host[k:k + 1].copy_(ws.view(torch.int32)[off.value:off.value + 1], non_blocking=True)
        return host

    @staticmethod
    def raise_input_flags(flags: Optional[torch.Tensor]) -> None:
        for flag in ([] if flags is None else flags.tolist()):
            if flag == 1:
                raise RuntimeError('molgym_hip error -1: charges: the real atoms of a canvas must be compacted to the front '
                                   '(a padding slot precedes an atom)')
            if flag == 2:
                raise RuntimeError('molgym_hip error -1: cfg.TA / cfg.TE do not match the atom counts in charges')
            if flag != 0:
                raise RuntimeError(f'molgym_hip error -1: list build reported error {flag}')

    def ppo_minibatch(self, batch: 'DeviceBatch', clip_ratio: float, vf_coef: float, entropy_coef: float,
                      loss_scale: float = 1.0, slot: int = 0, stats_accum: Optional[torch.Tensor] = None,
                      graph: Optional[bool] = None, epoch_cache: bool = False,
                      grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One compute_loss forward + backward (molgym/ppo.py:124-131) entirely on the device, ONE C call (mg_cov_ppo_step):
        step -> float64 PPO loss -> hand-written backward, gradients ACCUMULATED (atomically) into theta.grad.
        Returns the 6 float64 loss statistics (device tensor, no sync); `stats_accum` (6 float64, optional) additionally gets
        loss_scale x statistics added on the device (ppo.train's epoch mean without a tensor per mini-batch).  `slot` selects an
        independent workspace AND an independent cached graph, so the mini-batches of one epoch -- independent given theta --
        can be in flight on several HIP streams.  `graph` (default: on, MG_GRAPH=0 in the environment turns it off): the ~27
        launches of the step are recorded and issued as one hipGraph launch whose kernel nodes are updated in place
        (include/molgym_hip.h: the update loop is otherwise bound by the host's launch rate); the library falls back to plain
        stream launches where a graph cannot express the step.  `epoch_cache` (ppo.train's loop): theta is constant over the
        mini-batches of an epoch, so the derived weight matrices of this slot's workspace are prepared by the slot's FIRST
        mini-batch after `invalidate_weights()` only, and the expanded complex weight gradients stay in the workspace until
        `fold_gradients()` -- theta.grad is incomplete until then.  `grad_out` (flat float32, theta's size; default theta.grad)
        receives the gradient instead (ppo.train's ordered data-parallel mode: one row per mini-batch): the step then folds its
        expanded weight gradients itself, also with `epoch_cache` (which still spares the weight preparation), and the maxl < 4
        detour through the kernel-side buffer lands in `grad_out` too."""
        _refuse_deterministic('ppo_minibatch')
        ws = self._workspace(batch.cfg, slot, epoch_step=epoch_cache)
        flags = 0
        if epoch_cache:
            st = self._ws_epoch.setdefault(slot, {'weights': False, 'pending': False})
            if grad_out is None:
                flags = _lib.STEP_DEFER_FOLD | (_lib.STEP_WEIGHTS_CURRENT if st['weights'] else 0)
                st.update(weights=True, pending=True, cfg=batch.cfg)
            else:  # the row must be complete when the step returns: folded in the step, nothing left pending
                if st['pending']:
                    raise RuntimeError('ppo_minibatch(grad_out=...): this slot holds deferred weight gradients of earlier '
                                       'mini-batches (fold_gradients() first)')
                flags = _lib.STEP_WEIGHTS_CURRENT if st['weights'] else 0
                st.update(weights=True, cfg=batch.cfg)
        else:
            self._ws_epoch.pop(slot, None)  # (this call re-prepares the weights and zeroes the accumulator)

        def call(out, gout, stats, grad, graph_slot, used):
            theta_k = self._ktheta(refresh=not (flags & _lib.STEP_WEIGHTS_CURRENT))
            self._chk(self._L().mg_cov_ppo_step(C.byref(batch.cfg), ptr(theta_k), ptr(batch.pos), ptr(batch.charges),
                                                ptr(batch.bags), ptr(batch.actions), ptr(self.leb), ptr(ws), ws.numel(),
                                                ptr(batch.logp), ptr(batch.adv), ptr(batch.ret), clip_ratio, vf_coef, entropy_coef,
                                                float(loss_scale), ptr(out), ptr(gout), ptr(stats), ptr(stats_accum),
                                                ptr(self._kgrad(slot, grad)), graph_slot, flags, used, self._s()))

        stats = self._ppo_frame(batch, ws, slot, graph, grad_out, call)
        if not epoch_cache or grad_out is not None:
            self._kgrad_collect(slot, grad_out)  # (maxl < 4; with epoch_cache the gather follows the fold, fold_gradients)
        self._unchecked[slot] = (batch.cfg, ws)
        return stats

    def _step_sample(self, observations: List[ObservationType]) -> Dict[str, Any]:
        """step(obs) of the rollout (agent.py:229-292, ppo.py:188,205): draw the sub-actions on the device
        (training) or take the argmax variants (evaluation) and return logp / ent / v of what was drawn."""
        N = self.observation_space.canvas_space.size
        pos, charges, bags, natoms = parse_observations_host(observations, self.zs, N)
        B = len(observations)
        cfg = self._make_cfg(B, natoms)
        dev = self.theta.device
        d_pos, d_chg, d_bag = self._upload_packed(pos, charges, bags)
        ws = self._workspace(cfg)
        out = torch.empty(3, B, dtype=torch.float32, device=dev)
        acts = torch.empty(B, 6, dtype=torch.float32, device=dev)
        mode = 1 if self.training else 2
        with self._guard():
            self._chk(self._L().mg_cov_sample(C.byref(cfg), ptr(self._ktheta()), ptr(d_pos), ptr(d_chg), ptr(d_bag),
                                                ptr(self.leb), C.c_uint64(self.draw_seed()), mode, ptr(ws), ws.numel(),
                                                ptr(acts), ptr(out), self._s()))
        self._last_ws, self._last_cfg = ws, None
        self._unchecked.pop(0, None)  # slot 0's workspace now holds this sampling launch's lists
        dists = self._dists(cfg, ws, d_bag)
        with self._guard():  # this path synchronises for the actions anyway: surface the list build's error flags
            self._chk(self._L().mg_cov_check(C.byref(cfg), ptr(ws), ws.numel(), self._s()))
        host = acts.cpu().numpy()
        return {'actions': [self.to_action_space(a, o) for a, o in zip(host, observations)], 'a': acts,
                'logp': out[0], 'ent': out[1], 'v': out[2], 'dists': dists}

    # -- persistent device canvases (`make_canvas`): no per-step parse, the drawn atom is appended on the device -----------
    def _sample_canvas(self, canvas: 'DeviceCanvas', seed: Optional[int], sample_ids: Tuple[int, int], acts: torch.Tensor,
                       out: torch.Tensor):
        """the sampling launch of `step_canvas` alone (also `episodes.DeviceEpisodes.step`): draws the action rows `acts`
        (E, 6) and logp / ent / v `out` (3, E) on the resident canvases, sized by the host mirror of the atom counts; nothing
        is copied to the host.  Returns the launch's (cfg, workspace)."""
        cfg = self._make_cfg(canvas.E, canvas.natoms)
        ws = self._workspace(cfg)
        if seed is None:
            seed = self.draw_seed()
        mode = 1 if self.training else 2
        with self._guard():
            self._chk(self._L().mg_cov_sample_ids(C.byref(cfg), ptr(self._ktheta()), ptr(canvas.pos32), ptr(canvas.charges),
                                                    ptr(canvas.bags), ptr(self.leb), C.c_uint64(seed), int(sample_ids[0]),
                                                    int(sample_ids[1]), mode, ptr(ws), ws.numel(), ptr(acts), ptr(out),
                                                    self._s()))
        self._last_ws, self._last_cfg = ws, None
        self._unchecked.pop(0, None)
        return cfg, ws

    def check_launch(self, launch) -> None:
        """the list build of a sampling launch flags canvases that disagree with the host mirror in its workspace"""
        self._unchecked[0] = launch
        self.check_inputs()

    def step_canvas(self, canvas: 'DeviceCanvas', commit: bool = True, seed: Optional[int] = None,
                    sample_ids: Tuple[int, int] = (0, 1)) -> Dict[str, Any]:
        """step(observations) of the rollout on resident canvases: same sampling kernels, same return dict; with
        `commit` the drawn atoms are then placed on the canvases in HBM (the host hands `actions` to the environments
        and calls `canvas.sync` for the ones that were reset or changed in any other way).
        `seed` / `sample_ids = (base, stride)`: the random stream of canvas row b is keyed by (seed, base + stride * b) --
        a rollout stepped in groups of environments passes the step's common seed and the group's environment ids, and
        every environment draws what one call over all of them would draw (ppo._rollout_pipelined)."""
        B = canvas.E
        natoms_before = canvas.natoms.copy()
        dev = self.theta.device
        out = torch.empty(3, B, dtype=torch.float32, device=dev)
        acts = torch.empty(B, 6, dtype=torch.float32, device=dev)
        cfg, ws = self._sample_canvas(canvas, seed, sample_ids, acts, out)
        dists = self._dists(cfg, ws, canvas.bags.clone())
        newpos = canvas.append(acts, commit)
        host_a, host_p = acts.cpu().numpy(), newpos.cpu().numpy()  # the action rows and the positions they place
        elements = np.rint(host_a[:, 1]).astype(np.int64)
        if commit:
            canvas.commit_mirror(natoms_before, elements, host_p)
        actions = [(int(e), (float(p[0]), float(p[1]), float(p[2]))) for e, p in zip(elements, host_p)]
        return {'actions': actions, 'a': acts, 'logp': out[0], 'ent': out[1], 'v': out[2], 'dists': dists}

    def workspace_view(self, name: str, cfg: _lib.CovCfg) -> torch.Tensor:
        """float32 view of a named intermediate of the last forward (tests only)."""
        off, cnt = C.c_int64(), C.c_int64()
        self._chk(self._L().mg_cov_workspace_lookup(C.byref(cfg), name.encode(), C.byref(off), C.byref(cnt)))
        return self._last_ws.view(torch.float32)[off.value:off.value + cnt.value]

    def workspace_view_int(self, name: str, cfg: _lib.CovCfg) -> torch.Tensor:
        """int32 view of a named index list of the last forward (natoms, atom_off, err, ...)."""
        return self.workspace_view(name, cfg).view(torch.int32)
