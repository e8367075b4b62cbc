"""The ordered data-parallel mode of `ppo.train` (molgym_amd.set_deterministic(True, data_parallel=True)) on the host, no GPU:

* `shard_epoch_whole`: every mini-batch whole, exactly once, at rank k % world, at the row the fold kernel reads it from;
* the third switch: keyword semantics, MG_DP_ORDERED, the three RuntimeErrors of `train`, no warning while it is on;
* a float32 stand-in agent on the CPU (the interface `train` takes its device path on, plus `grad_out=` and
  `fold_minibatch_rows` in plain torch, sequentially in k order) trained over gloo at world 1, 2, 3 and 4 with M = 4 and M = 3
  mini-batches (world 4, M = 3: one rank owns nothing), in the run-ahead and in the synchronous loop, with an even and an odd
  parameter count (the statistics field of a row 8-byte aligned or not): theta, optimizer state and infos are torch.equal / ==
  across all worlds and ranks;
* one collective per epoch, counted through a wrapper.
The stand-in's per-sample gradients spread over six decades, so that the order of the float32 additions shows."""
import logging
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from molgym_amd import ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 8


# ---- the partition ---------------------------------------------------------------------------------------------------------
def test_shard_epoch_whole_deals_every_minibatch_whole_to_rank_k_mod_world():
    from molgym_amd import _lib
    for M in range(10):
        n = max(M * MB - 3, 0)  # (M - 1 full mini-batches and a ragged one of 5)
        batches = list(ppo.get_batch_generator(np.arange(n), MB))
        assert len(batches) == M
        for world in range(1, 6):
            per_rank = -(-M // world)
            seen, rows = {}, set()
            for rank in range(world):
                work = ppo.shard_epoch_whole(batches, rank, world)
                assert len(work) <= per_rank
                for j, (idx, share) in enumerate(work):
                    k = j * world + rank  # this rank's j-th mini-batch is global mini-batch k
                    assert share == 1.0 and k < M and k % world == rank
                    assert np.array_equal(idx, batches[k])  # whole, the ragged last one included
                    assert k not in seen
                    seen[k] = rank
                    # row j of rank `rank` among the gathered [world][per_rank] rows is where the fold looks for k
                    row = _lib.fold_row_index(k, world, per_rank)
                    assert row == rank * per_rank + j == (k % world) * per_rank + k // world
                    rows.add(row)
            assert sorted(seen) == list(range(M)) and len(rows) == M
            assert all(r < world * per_rank for r in rows)


def test_row_layout():
    from molgym_amd import _lib
    for n in (0, 1, 3, 4, 5, 255, 1027, 185006, 212524):
        rb = _lib.fold_row_bytes(n)
        assert rb % 16 == 0 and n * 4 + 48 <= rb < n * 4 + 48 + 16


# ---- the switch ------------------------------------------------------------------------------------------------------------
def _child(code, **env):
    e = dict(os.environ)
    for k in ('MG_DETERMINISTIC', 'MG_COV_ORDERED', 'MG_DP_ORDERED'):
        e.pop(k, None)
    e.update(env)
    return subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def test_keyword_semantics(built_lib):
    r = _child('import molgym_amd as m\n'
               'assert m.is_deterministic_data_parallel() is False\n'
               'm.set_deterministic(True, data_parallel=True)\n'
               'assert m.is_deterministic() and m.is_deterministic_data_parallel() and not m.is_deterministic_covariant()\n'
               'm.set_deterministic(True)\n'  # every call without the keyword turns it off
               'assert m.is_deterministic() and not m.is_deterministic_data_parallel()\n'
               'm.set_deterministic(True, covariant=True, data_parallel=True)\n'
               'assert m.is_deterministic_covariant() and m.is_deterministic_data_parallel()\n'
               'm.set_deterministic(True, covariant=True)\n'
               'assert m.is_deterministic_covariant() and not m.is_deterministic_data_parallel()\n'
               'm.set_deterministic(False, data_parallel=True)\n'  # `on and data_parallel`
               'assert not m.is_deterministic() and not m.is_deterministic_data_parallel()\n'
               'print("ok")')
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr


def test_environment_turns_it_on(built_lib):
    code = 'import molgym_amd as m\nprint(int(m.is_deterministic_data_parallel()))'
    for value, want in (('1', '1'), ('0', '0'), ('', '0')):
        r = _child(code, MG_DP_ORDERED=value)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


# ---- the stand-in agent ----------------------------------------------------------------------------------------------------
class _Rollout:
    def __init__(self, data):
        self.data = data

    def minibatch(self, indices, idx_dev=None):
        return ppo.collect_data_batch(self.data, np.asarray(indices))


class StandIn(torch.nn.Module):
    """what `ppo.train` calls on the HIP agents, in float32 torch on the CPU.  An observation is a row of three feature vectors
    whose entries are normal x 10^uniform(-3, 3): the per-sample gradients spread over six decades in every parameter."""
    flat_gradient_on_host = True

    def __init__(self, P):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.theta = torch.nn.Parameter(torch.randn(P, generator=g) * 0.5)

    def step(self, observations, actions=None):
        X = torch.as_tensor(np.asarray(observations), dtype=torch.float32)  # [B, 3, P]
        z = (X * 1e-3) @ self.theta
        return {'logp': -1.0 + 0.1 * torch.tanh(z[:, 0]), 'ent': 1.0 + 0.1 * torch.tanh(z[:, 1]), 'v': z[:, 2]}

    def prepare_rollout(self, data):
        return _Rollout(data)

    def ppo_minibatch(self, batch, clip_ratio, vf_coef, entropy_coef, loss_scale=1.0, slot=0, stats_accum=None, grad_out=None):
        loss, info = ppo.compute_loss(self, batch, clip_ratio, vf_coef, entropy_coef)
        g, = torch.autograd.grad(loss * loss_scale, self.theta)
        if grad_out is None:
            if self.theta.grad is None:
                self.theta.grad = torch.zeros_like(self.theta)
            grad_out = self.theta.grad
        assert grad_out.dtype == torch.float32 and grad_out.shape == g.shape
        grad_out += g
        stats = torch.tensor([info[k] for k in ppo.KEYS], dtype=torch.float64)
        stats_accum += stats * loss_scale
        return stats

    def fold_minibatch_rows(self, rows, world, per_rank, total, grad_out=None, stats_out=None):
        """mg_fold_rows in plain torch: sequentially in k order, from +0"""
        P = self.theta.numel()
        assert rows.dtype == torch.uint8 and rows.shape[0] == world * per_rank and rows.shape[1] % 16 == 0
        g, s = torch.zeros(P, dtype=torch.float32), torch.zeros(6, dtype=torch.float64)
        for k in range(total):
            r = rows[(k % world) * per_rank + k // world]
            g = g + r[:P * 4].view(torch.float32)
            s = s + r[P * 4:P * 4 + 48].clone().view(torch.float64)  # (clone: the field may sit at a 4-byte boundary)
        (self.theta.grad if grad_out is None else grad_out).copy_(g)
        if stats_out is not None:
            stats_out.copy_(s)

    def grad_norm_clip(self, max_norm=0.0):
        norm = torch.norm(self.theta.grad, 2)
        if max_norm > 0:
            coef = max_norm / (norm + 1e-6)
            if coef < 1:
                self.theta.grad.mul_(coef)
        return norm.reshape(1)

    def ppo_epoch_end(self, max_norm, stats_accum, num_minibatches, kl_limit, rec, stop_flag):
        stats = stats_accum / max(int(num_minibatches), 1)
        stop = bool(stop_flag.item()) or stats[4].item() > kl_limit
        norm = self.grad_norm_clip(0.0 if stop else max_norm)
        rec[:6] = stats
        rec[6] = norm.double()
        rec[7] = 1.0 if stop else 0.0
        if stop:
            stop_flag.fill_(1)

    def adam_supported(self, optimizer):
        return True

    def adam_step(self, optimizer, skip_flag=None):
        if skip_flag is None or skip_flag.item() == 0:
            optimizer.step()
        return True

    def adam_unstep(self, optimizer, count):
        pass


def _data(n, P):
    rng = np.random.default_rng(100 + n + P)
    obs = (rng.standard_normal((n, 3, P)) * 10.0 ** rng.uniform(-3, 3, (n, 3, P))).astype(np.float32)
    d = dict(obs=obs, act=np.zeros((n, 1)), adv=rng.standard_normal(n), ret=rng.standard_normal(n))
    with torch.no_grad():
        d['logp'] = StandIn(P).step(obs)['logp'].double().numpy() + 0.01
    return d


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


CASES = [(P, n, runahead) for P in (40, 37) for n in (30, 20) for runahead in (True, False)]  # n = 30 / 20: M = 4 / 3


def _worker(rank, world, port, out):
    import torch.distributed as dist
    import molgym_amd
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    molgym_amd.set_deterministic(True, data_parallel=True)
    counts = {}

    def counted(name):
        fn = getattr(dist, name)

        def wrapper(*a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a, **kw)
        setattr(dist, name, wrapper)

    for name in ('all_gather', 'all_gather_into_tensor', 'all_reduce', 'broadcast', 'reduce', 'all_to_all', 'gather'):
        counted(name)
    warnings = []

    class Catch(logging.Handler):
        def emit(self, record):
            if record.levelno >= logging.WARNING:
                warnings.append(record.getMessage())

    logging.getLogger().addHandler(Catch())
    results = []
    for P, n, runahead in CASES:
        os.environ['MOLGYM_RUNAHEAD'] = '1' if runahead else '0'
        ac = StandIn(P)
        opt = torch.optim.Adam(ac.parameters(), lr=3e-2)
        np.random.seed(5)
        counts.clear()
        infos = ppo.train(ac, opt, _data(n, P), mini_batch_size=MB, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5,
                          entropy_coef=0.01, gradient_clip=0.5, max_num_steps=3)
        st = opt.state[ac.theta]
        results.append({'theta': ac.theta.detach().clone(), 'exp_avg': st['exp_avg'].clone(), 'exp_avg_sq': st['exp_avg_sq'].clone(),
                        'step': float(st['step']), 'infos': {k: v for k, v in infos.items() if k != 'time'},
                        'counts': dict(counts), 'rng_pos': np.random.get_state()[2]})
    torch.save({'results': results, 'warnings': warnings, 'warned': ppo._warned_deterministic_dp}, f'{out}.w{world}.r{rank}.pt')
    dist.destroy_process_group()


def test_same_bits_at_world_1_2_3_4_in_both_loops_and_one_collective_per_epoch(built_lib, tmp_path):
    out = str(tmp_path / 'run')
    for world in (1, 2, 3, 4):
        mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    runs = {(w, r): torch.load(f'{out}.w{w}.r{r}.pt', weights_only=False) for w in (1, 2, 3, 4) for r in range(w)}
    base = runs[(1, 0)]['results']
    for c, (P, n, runahead) in enumerate(CASES):
        a = base[c]
        assert a['infos']['num_opt_steps'] == 3 and a['step'] == 3.0
        assert torch.isfinite(a['theta']).all() and not torch.equal(a['theta'], StandIn(P).theta.detach())
        for (w, r), run in runs.items():
            b = run['results'][c]
            for k in ('theta', 'exp_avg', 'exp_avg_sq'):
                assert torch.equal(a[k], b[k]), (P, n, runahead, w, r, k)
            assert a['step'] == b['step'] and a['rng_pos'] == b['rng_pos']
            assert set(a['infos']) == set(b['infos'])
            for k in a['infos']:
                assert a['infos'][k] == b['infos'][k], (P, n, runahead, w, r, k)
            # ONE gather per epoch replaces both all-reduces (world 1: none at all); one broadcast per call (the permutations)
            want = {'broadcast': 1} if w == 1 else {'broadcast': 1, 'all_gather': 3}
            assert b['counts'] == want, (w, r, b['counts'])
    for run in runs.values():
        assert run['warnings'] == [] and run['warned'] is False  # `reproducible within a rank only` is not said in this mode


def test_the_order_matters_for_the_stand_in(built_lib):
    """control: with these gradients the fold in reversed k order gives other bits -- an all-reduce could not pass the test above"""
    P, n = 40, 30
    ac, data = StandIn(P), _data(n, P)
    rows = []
    for lo in range(0, n, MB):
        g, acc = torch.zeros(P), torch.zeros(6, dtype=torch.float64)
        ac.ppo_minibatch(ppo.collect_data_batch(data, np.arange(lo, min(lo + MB, n))), 0.2, 0.5, 0.01, stats_accum=acc, grad_out=g)
        rows.append(g)
    fwd, rev = torch.zeros(P), torch.zeros(P)
    for k in range(len(rows)):
        fwd, rev = fwd + rows[k], rev + rows[len(rows) - 1 - k]
    assert (fwd != rev).float().mean().item() >= 0.1


# ---- what `train` refuses --------------------------------------------------------------------------------------------------
class CovariantAC(StandIn):
    """(the name is what `train` goes by)"""


class OnlyStep(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(2, 3)


def test_train_raises_without_what_the_mode_stands_on(built_lib, monkeypatch):
    import molgym_amd
    from molgym_amd import _lib
    prev = (_lib.is_deterministic(), _lib.is_deterministic_covariant(), _lib.is_deterministic_data_parallel())
    kw = dict(mini_batch_size=MB, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01, gradient_clip=0.5, max_num_steps=2)
    try:
        data = _data(20, 40)
        # the first switch is off (the environment, or the C call, can leave the third one on alone)
        molgym_amd.set_deterministic(False)
        monkeypatch.setattr(_lib, '_dp_ordered', True)
        ac = StandIn(40)
        with pytest.raises(RuntimeError, match='deterministic mode is off'):
            ppo.train(ac, torch.optim.Adam(ac.parameters()), data, **kw)
        # CovariantAC without its own ordered mode
        molgym_amd.set_deterministic(True, data_parallel=True)
        ac = CovariantAC(40)
        with pytest.raises(RuntimeError, match='covariant=True'):
            ppo.train(ac, torch.optim.Adam(ac.parameters()), data, **kw)
        # an agent without the device path
        ac = OnlyStep()
        with pytest.raises(RuntimeError, match='device path'):
            ppo.train(ac, torch.optim.Adam(ac.parameters()), data, **kw)
        # and with everything in place it trains
        ac = StandIn(40)
        infos = ppo.train(ac, torch.optim.Adam(ac.parameters()), data, **kw)
        assert infos['num_opt_steps'] == 2
        # switch off: the stand-in trains on the old path, untouched by the new arguments
        molgym_amd.set_deterministic(True)
        ac = StandIn(40)
        assert ppo.train(ac, torch.optim.Adam(ac.parameters()), data, **kw)['num_opt_steps'] == 2
    finally:
        _lib.set_deterministic(prev[0], covariant=prev[1], data_parallel=prev[2])
