"""Workload for a kernel + memory-copy trace of SchNetAC.step_canvas (GPU box), and the per-step copy count read off that trace.
usage: rocprofv3 --kernel-trace --hip-runtime-trace --memory-copy-trace --output-format csv -d DIR -o int_canvas -- \
           python tools/int_canvas_trace.py [steps] [batch]
       python tools/int_canvas_trace.py --count DIR     (copies and synchronising calls between consecutive k_int_assemble)"""
import csv
import glob
import os
import sys

sys.path.insert(0, '.')


def run(steps, B):
    import torch
    from molgym_amd.agents.internal import SchNetAC
    from molgym_amd.spaces import ActionSpace, ObservationSpace
    from molgym_amd.synthetic import CONFIGS, make_batch
    cfg = CONFIGS['cfg2']
    torch.manual_seed(0)
    ac = SchNetAC(ObservationSpace(cfg['canvas_size'], cfg['zs']), ActionSpace(cfg['zs']), (0.8, 1.8), 128, device='cuda:0')
    ac.training = True
    obs = make_batch(B, cfg['canvas_size'], cfg['zs'], seed=0)['obs']
    canvas = ac.make_canvas(obs)
    with torch.no_grad():
        for _ in range(steps):
            ac.step_canvas(canvas, commit=False)
    torch.cuda.synchronize()
    print(f'{steps} step_canvas calls, B={B}')


def _rows(path):
    with open(path, newline='') as f:
        return list(csv.DictReader(f))


def _col(row, *names):
    low = {k.lower(): v for k, v in row.items()}
    for n in names:
        if n.lower() in low:
            return low[n.lower()]
    raise KeyError(names)


def count(d):
    """per step (window between two consecutive k_int_assemble launches, in host time through the HIP API records): the
    memory-copy API calls and the synchronising calls the step made, and the copies the memory-copy trace recorded"""
    find = lambda pat: sorted(glob.glob(os.path.join(d, '**', pat), recursive=True))
    kt, at, mt = find('*kernel_trace.csv'), find('*hip_api_trace.csv'), find('*memory_copy_trace.csv')
    if not kt or not at:
        print('need the kernel trace and the HIP runtime API trace under', d)
        return 1
    corr = {_col(r, 'Correlation_Id') for r in _rows(kt[0]) if 'k_int_assemble' in _col(r, 'Kernel_Name')}
    api = [(int(_col(r, 'Start_Timestamp')), _col(r, 'Function'), _col(r, 'Correlation_Id')) for r in _rows(at[0])]
    starts = sorted(t for t, _, c in api if c in corr)
    copies = [] if not mt else [(int(_col(r, 'Start_Timestamp')), _col(r, 'Direction')) for r in _rows(mt[0])]
    print(f'{len(starts)} steps (k_int_assemble launches); per step, between two of them:')
    for i in range(len(starts) - 1):
        calls = [f for t, f, _ in api if starts[i] <= t < starts[i + 1]]
        mem = [f for f in calls if 'Memcpy' in f]
        sync = [f for f in calls if 'Synchronize' in f]
        launches = sum('LaunchKernel' in f or 'ExtModuleLaunchKernel' in f for f in calls)
        dirs = [dr for t, dr in copies if starts[i] <= t < starts[i + 1]]
        h2d, d2h = sum('HOST_TO_DEVICE' in x for x in dirs), sum('DEVICE_TO_HOST' in x for x in dirs)
        print(f'step {i}: memory-copy API calls {len(mem)} {sorted(set(mem))}, synchronising calls {len(sync)}, kernel launches '
              f'{launches}; memory-copy trace: host-to-device {h2d}, device-to-host {d2h}')
    return 0


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--count':
        sys.exit(count(sys.argv[2]))
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 12, int(sys.argv[2]) if len(sys.argv) > 2 else 140)
