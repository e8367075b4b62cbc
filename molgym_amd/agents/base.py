"""Actor-critic interface (mirror of /root/reference/molgym/agents/base.py:10-19) and what the two HIP agents share:
ONE flat float32 parameter vector `theta` whose named slots are the reference module's state_dict entries."""
import abc
import ctypes as C
import functools
from collections import OrderedDict
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib

try:
    from torch.nn.modules.module import _IncompatibleKeys
except ImportError:  # pragma: no cover
    from collections import namedtuple
    _IncompatibleKeys = namedtuple('IncompatibleKeys', ['missing_keys', 'unexpected_keys'])


def check_action_rows(acts, B: int, cols: int, focus_col: int, element_col: int, N: int, Z: int) -> np.ndarray:
    """the action rows as a contiguous float32 (B, cols) array, with to_one_hot's scatter_ error for a row whose focus is not in
    0..N-1 or whose element is not in 0..Z-1 (a NaN is in neither); an empty batch passes"""
    acts = np.ascontiguousarray(np.asarray(acts, dtype=np.float32))
    assert acts.shape == (B, cols)
    focus, element = np.rint(acts[:, focus_col]), np.rint(acts[:, element_col])
    if B and not (focus.min() >= 0 and focus.max() < N and element.min() >= 0 and element.max() < Z):
        raise RuntimeError('index out of range in one-hot selection')
    return acts


class AbstractActorCritic(torch.nn.Module, abc.ABC):
    def __init__(self, observation_space, action_space):
        super().__init__()
        self.observation_space = observation_space
        self.action_space = action_space

    @abc.abstractmethod
    def step(self, observations: List, actions: Optional[np.ndarray] = None) -> dict:
        raise NotImplementedError

    def evaluate_actions(self, observations: List, actions: np.ndarray) -> dict:
        """Action evaluation under the name BASELINE.json's north_star uses; the reference spells it
        step(observations, actions) (base.py:17-19, ppo.py:26)."""
        return self.step(observations, actions)


class FlatThetaAgent(AbstractActorCritic):
    """`self.theta` (nn.Parameter, flat) + `self.slot_table` (name -> (offset, shape), molgym_amd/layout.py).

    state_dict() / load_state_dict() speak the REFERENCE module's keys -- one entry per tensor the reference agent
    registers (covariant/agent.py:58-143, internal/agent.py:37-105) -- so a checkpoint written through state_dict()
    by either implementation loads into the other; the flat vector itself is accepted too ({'theta': ...}).
    Whole-module pickling (ModelIO, tools/model_util.py:82-100) keeps working: only caches are dropped."""

    # entries of a reference checkpoint that carry no trainable state of this path (cormorant's fixed cut-off
    # parameters and zero buffers, the agents' index helper buffers)
    _IGNORED_SUFFIXES = ('soft_cut_rad', 'soft_cut_width', 'zero', 'channel_offsets', 'zs_tensor', 'leb')
    action_cols = None  # columns of an action row (subclasses: 6 / 7)
    # ppo_minibatch issues its launches as one updated hipGraph launch (include/molgym_hip.h: mg_cov_ppo_step, mg_int_ppo_step)
    use_graphs = True
    # caches and the records of the last call, (name, constructor of the empty value or None): plain attributes that are never
    # pickled and are empty after __init__ and __setstate__.  `_ws_cache`: the cached blocks of `_cached_block` (a step
    # workspace per slot); `_ws_epoch`: per slot, what its workspace holds of the current PPO epoch
    _TRANSIENT = (('_ws_cache', dict), ('_ws_epoch', dict), ('_last_ws', None), ('_last_cfg', None), ('_last_out', None),
                  ('_last_gout', None), ('last_step_used_graph', bool))

    def __init__(self, observation_space, action_space):
        super().__init__(observation_space, action_space)
        self._reset_transient()

    def _reset_transient(self) -> None:
        for name, empty in self._TRANSIENT:
            setattr(self, name, empty and empty())

    # (an instance that lacks `_ws_epoch` -- tests take it out of one to forget an epoch -- finds an empty one at its next use)
    _ws_epoch = functools.cached_property(lambda self: {})

    # whole-module pickling (ModelIO.save = torch.save(module), tools/model_util.py:82-91) drops the caches; a pickle of an
    # earlier version holds some of them or none
    def __getstate__(self):
        state = self.__dict__.copy()
        for name, _ in self._TRANSIENT:
            state.pop(name, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._reset_transient()

    def _slot(self, name: str, tensor: Optional[torch.Tensor] = None) -> torch.Tensor:
        off, shape = self.slot_table[name]
        t = self.theta if tensor is None else tensor
        return t[off:off + int(np.prod(shape))].view(shape)

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """Named CLONES with the reference module's state_dict keys."""
        t = self.theta.detach()
        return {k: self._slot(k, t).clone() for k in self.slot_table}

    def import_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        with torch.no_grad():
            for k in self.slot_table:
                self._slot(k).copy_(sd[k].to(self.theta).reshape(self.slot_table[k][1]))

    def state_dict(self, *args, destination=None, prefix='', keep_vars=False):
        if args:  # the legacy positional form (destination, prefix, keep_vars) torch.nn.Module still accepts
            destination = args[0] if destination is None else destination
            prefix = args[1] if len(args) > 1 and prefix == '' else prefix
            keep_vars = args[2] if len(args) > 2 and keep_vars is False else keep_vars
        out = OrderedDict() if destination is None else destination
        t = self.theta if keep_vars else self.theta.detach()
        for k in self.slot_table:
            out[prefix + k] = self._slot(k, t)
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sd = dict(state_dict)
        if set(sd) == {'theta'}:
            with torch.no_grad():
                self.theta.copy_(sd['theta'].to(self.theta).reshape(-1))
            return _IncompatibleKeys([], [])
        missing = [k for k in self.slot_table if k not in sd]
        unexpected = [k for k in sd if k not in self.slot_table and not k.endswith(self._IGNORED_SUFFIXES)]
        bad = [k for k, (_, s) in self.slot_table.items() if k in sd and tuple(sd[k].shape) != tuple(s)]
        if bad:
            raise RuntimeError('size mismatch for ' + ', '.join(
                f'{k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(self.slot_table[k][1])}' for k in bad))
        if strict and (missing or unexpected):
            raise RuntimeError(f'Error(s) in loading state_dict for {type(self).__name__}: missing keys {missing}, '
                               f'unexpected keys {unexpected}')
        with torch.no_grad():
            for k in self.slot_table:
                if k in sd:
                    self._slot(k).copy_(sd[k].to(self.theta))
        return _IncompatibleKeys(missing, unexpected)

    # -- device plumbing ----------------------------------------------------------------------------------------------
    def _upload_packed(self, *arrays: np.ndarray) -> List[torch.Tensor]:
        """ONE host -> device copy for several 4-byte-typed (float32 / int32) arrays: packed into one host buffer, sections
        aligned to 256 bytes, returned as typed device views of the arrays' shapes (one H2D per batch; four
        separate pageable copies cost four synchronous transfers)."""
        assert all(x.dtype.itemsize == 4 for x in arrays), [x.dtype for x in arrays]
        offs, total = _lib.sections([x.size for x in arrays], 64)
        host = np.empty(max(total, 64), dtype=np.int32)
        for x, o in zip(arrays, offs):
            host[o:o + x.size] = np.ascontiguousarray(x).reshape(-1).view(np.int32)
        dev = torch.from_numpy(host).to(self.theta.device)
        out = []
        for x, o in zip(arrays, offs):
            v = dev[o:o + x.size]
            out.append((v.view(torch.float32) if x.dtype == np.float32 else v).view(x.shape))
        return out

    def _f64(self, x):
        """`x` on the agent's device as float64 (the loss inputs logp / adv / ret): a tensor is moved, anything else uploaded;
        None stays None"""
        if x is None:
            return None
        if torch.is_tensor(x):
            return x.to(self.theta.device, torch.float64)
        return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(self.theta.device)

    def _guard(self):
        """Every C call runs with the agent's device current: the library keeps per-device state (CG tables in
        __constant__ memory, function attributes, side stream) keyed by hipGetDevice()."""
        return torch.cuda.device(self.theta.device)

    def _s(self):
        """torch's current stream ON THE AGENT'S DEVICE (not on whatever device happens to be current)"""
        return C.c_void_p(torch.cuda.current_stream(self.theta.device).cuda_stream)

    def _require_device(self) -> None:
        if self.theta.device.type != 'cuda':
            raise RuntimeError(f'{type(self).__name__} runs on the HIP device only (no CPU fallback)')

    def _cached_block(self, key, nbytes: int):
        """(block, replaced): the uint8 block cached under `key` in `_ws_cache` if it holds `nbytes` on this device, otherwise
        a new one with a quarter of headroom in its place (the caller deals with what the old one still held first)"""
        ws = self._ws_cache.get(key)
        if ws is not None and ws.numel() >= nbytes and ws.device == self.theta.device:
            return ws, False
        ws = self._ws_cache[key] = torch.empty(int(nbytes * 1.25), dtype=torch.uint8, device=self.theta.device)
        return ws, True

    # -- what the rollout and the update ask of either agent ----------------------------------------------------------------
    @staticmethod
    def draw_seed() -> int:
        """one sampling seed from the torch RNG (follows torch.manual_seed, util.set_seeds)"""
        return int(torch.randint(0, 2**62, (1, )).item())

    def make_canvas(self, observations: List):
        """persistent device canvases (rollouts): no per-step parse, the drawn atom is placed on the device (agents/canvas.py)"""
        from .canvas import DeviceCanvas
        return DeviceCanvas(self, observations)

    def check_launch(self, launch) -> None:
        """raise what the sampling launch `launch` (what `_sample_canvas` returned) flagged on the device: nothing here"""

    def _ppo_frame(self, batch, ws: torch.Tensor, slot: int, graph: Optional[bool], grad_out: Optional[torch.Tensor], call) -> torch.Tensor:
        """What `ppo_minibatch` is around either agent's C call: the step's output buffers, the gradient target (`grad_out`,
        checked, or theta.grad, created if need be), the choice between graph and stream launches and the record of the call
        (`_last_*`, `last_step_used_graph`).  `call(out, gout, stats, grad, graph_slot, used)` issues the launches under the
        device guard.  Returns the 6 float64 statistics."""
        theta, B = self.theta, batch.cfg.B
        out = torch.empty(3, B, dtype=torch.float32, device=theta.device)
        gout = torch.empty(3, B, dtype=torch.float32, device=theta.device)
        stats = torch.empty(6, dtype=torch.float64, device=theta.device)
        if grad_out is None:
            if theta.grad is None:
                theta.grad = torch.zeros_like(theta)
            grad_out = theta.grad
        else:
            assert grad_out.dtype == torch.float32 and grad_out.numel() == theta.numel() and grad_out.is_contiguous() and \
                grad_out.device == theta.device
        use_graph = self.use_graphs if graph is None else graph
        used = C.c_int32(0)
        with self._guard():
            call(out, gout, stats, grad_out, slot if use_graph else -1, C.byref(used))
        self._last_ws, self._last_cfg, self._last_out, self._last_gout = ws, batch.cfg, out, gout
        self.last_step_used_graph = bool(used.value)
        return stats

    def adam_supported(self, optimizer) -> bool:
        """whether `adam_step` takes this optimizer (a plain torch.optim.Adam over the single flat theta, no step hooks)"""
        if type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
            return False
        # step hooks registered on the optimizer (or globally) must run: leave those cases to optimizer.step()
        from torch.optim import optimizer as _opt_mod
        if getattr(optimizer, '_optimizer_step_pre_hooks', None) or getattr(optimizer, '_optimizer_step_post_hooks', None) or \
                getattr(_opt_mod, '_global_optimizer_pre_hooks', None) or getattr(_opt_mod, '_global_optimizer_post_hooks', None):
            return False
        g = optimizer.param_groups[0]
        p = self.theta
        if len(g['params']) != 1 or g['params'][0] is not p or p.grad is None or not p.is_cuda:
            return False
        if g.get('capturable') or g.get('fused') or g.get('differentiable') or torch.is_tensor(g['lr']):
            return False
        if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse or not p.grad.is_contiguous():
            return False
        if g['amsgrad'] and len(optimizer.state[p]) and 'max_exp_avg_sq' not in optimizer.state[p]:
            return False
        return True

    def adam_step(self, optimizer, skip_flag: Optional[torch.Tensor] = None) -> bool:
        """optimizer.step() (ppo.py:145) for a plain torch.optim.Adam over the flat theta as ONE HIP launch (mg_adam_step)
        on the optimizer's own state tensors, which are created exactly as torch creates them -- so state_dict(), learning-
        rate schedulers (their step counter is advanced here) and a later optimizer.step() see nothing unusual; an
        optimizer with step hooks is left to optimizer.step().  Returns False (nothing done) for anything else:
        another optimizer class, several parameter groups / tensors, fused / capturable / differentiable variants.
        `skip_flag` (device int32, optional): the launch does nothing when it is non-zero (mg_adam_step_gated: the KL test of
        ppo.train taken on the device); the optimizer's step counter is advanced either way -- the caller takes the skipped
        steps back (`adam_unstep`) once it has read the flag."""
        if not self.adam_supported(optimizer):
            return False
        g = optimizer.param_groups[0]
        p = self.theta
        st = optimizer.state[p]
        if len(st) == 0:  # torch.optim.Adam._init_group
            st['step'] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if g['amsgrad']:
                st['max_exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if g['amsgrad'] and 'max_exp_avg_sq' not in st:
            return False
        st['step'] += 1
        step = int(st['step'].item()) if torch.is_tensor(st['step']) else int(st['step'])
        beta1, beta2 = g['betas']
        ptr = _lib.ptr
        with self._guard():
            _lib.check(_lib.lib().mg_adam_step_gated(p.numel(), ptr(p.data), ptr(p.grad), ptr(st['exp_avg']), ptr(st['exp_avg_sq']),
                                                     ptr(st['max_exp_avg_sq'] if g['amsgrad'] else None), float(g['lr']),
                                                     float(beta1), float(beta2), float(g['eps']), float(g['weight_decay']), step,
                                                     1 if g.get('maximize') else 0, ptr(skip_flag), self._s()))
        # what a learning-rate scheduler's wrapper of optimizer.step() would have recorded (lr_scheduler.py: `_step_count`,
        # `_opt_called`; the scheduler warns about "lr_scheduler.step() before optimizer.step()" otherwise)
        if hasattr(optimizer, '_step_count'):
            optimizer._step_count += 1
        optimizer._opt_called = True
        return True

    def adam_unstep(self, optimizer, count: int) -> None:
        """take back `count` optimizer steps whose launches the device-side gate skipped (step counters only: the parameters
        and moments were never touched)"""
        if count <= 0:
            return
        st = optimizer.state[self.theta]
        st['step'] -= count
        if hasattr(optimizer, '_step_count'):
            optimizer._step_count -= count

    def ppo_epoch_end(self, max_norm: float, stats_accum: torch.Tensor, num_minibatches: int, kl_limit: float,
                      rec: torch.Tensor, stop_flag: torch.Tensor) -> None:
        """mg_ppo_epoch_end: KL test, gradient norm and clip of one PPO epoch on the device (ppo.py:133-144); `rec` (8 float64)
        receives the epoch's statistics, the pre-clip norm and the state of the latching `stop_flag` (int32)."""
        scratch = torch.empty(1, dtype=torch.float32, device=self.theta.device)
        ptr = _lib.ptr
        with self._guard():
            _lib.check(_lib.lib().mg_ppo_epoch_end(self.theta.numel(), ptr(self.theta.grad), float(max_norm), ptr(stats_accum),
                                                   1.0 / max(int(num_minibatches), 1), float(kl_limit), ptr(rec), ptr(stop_flag),
                                                   ptr(scratch), self._s()))

    def fold_minibatch_rows(self, rows: torch.Tensor, world: int, per_rank: int, total: int,
                            grad_out: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None) -> None:
        """mg_fold_rows: `rows` (uint8, [world * per_rank, row bytes], rank-major as gathered; a row is [P float32 gradient | 6
        float64 statistics | pad to 16 bytes], `_lib.fold_row_bytes`) added up in global mini-batch order -- global mini-batch k
        sits at row `_lib.fold_row_index(k, world, per_rank)`, k < total; padding rows are not read.  `grad_out` (default:
        theta.grad) and `stats_out` (6 float64) are overwritten."""
        grad_out = self.theta.grad if grad_out is None else grad_out
        n = grad_out.numel()
        assert rows.dtype == torch.uint8 and rows.dim() == 2 and rows.is_contiguous() and rows.shape[0] == world * per_rank
        assert grad_out.dtype == torch.float32 and grad_out.is_contiguous() and grad_out.device == rows.device
        assert stats_out is None or (stats_out.dtype == torch.float64 and stats_out.numel() == 6 and stats_out.is_contiguous())
        with self._guard():
            _lib.check(_lib.lib().mg_fold_rows(n, int(world), int(per_rank), int(total), _lib.ptr(rows), int(rows.shape[1]),
                                               _lib.ptr(grad_out), _lib.ptr(stats_out), self._s()))

    def grad_norm_clip(self, max_norm: float = 0.0) -> torch.Tensor:
        """||theta.grad||_2 as a 1-element device tensor (util.compute_gradient_norm, tools/util.py:61-69) and, if
        max_norm > 0, theta.grad *= min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_, ppo.py:144) -- one C call on
        the flat gradient instead of ~60 per-tensor kernels."""
        norm = torch.empty(2, dtype=torch.float32, device=self.theta.device)
        with self._guard():
            _lib.check(_lib.lib().mg_grad_norm_clip(self.theta.numel(), _lib.ptr(self.theta.grad), float(max_norm),
                                                    _lib.ptr(norm), self._s()))
        return norm[:1]
