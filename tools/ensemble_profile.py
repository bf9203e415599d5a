#!/usr/bin/env python
"""Ensemble sweeps against what a user does without them.

Seeded inputs from bench.make_inputs; needs a GPU.  Times the bench C2 sweep (360 x 500 gates, one sub-beam) and one C4 sweep
(360 x 500, 7 x 7 sub-beams) with device-resident outputs:

  A  simulate_rays_ensemble for M in --members (default 1, 8, 32) with form='shared', and both forms at M = --m-b;
  B  M = --m-b separate RadarOperators, each with its own cube and tables, simulate_rays one after the other
     (runs unchanged on a commit without ensembles: --only-b).

A and B alternate in one process and the whole thing is repeated --repeat times (the spread); every window is at least
--window seconds of device work, closed by the context's synchronize.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/ensemble_profile.py --trace` (a few untimed sweeps of each kind).

  python tools/ensemble_profile.py --out profiles/ensemble_profile.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V']


def member_cubes(cube, n):
    """n states of the model: the cube, then seeded rescalings of its hydrometeor masses (three distinct host cubes used in
    turn: every member still gets a device cube of its own)."""
    rng = np.random.default_rng(7)
    out = [cube['data']]
    for _ in range(min(n - 1, 3)):
        d = dict(cube['data'])
        for k in d:
            if k.startswith('Q') and k.endswith('_v'):
                d[k] = (d[k] * np.float32(rng.uniform(0.5, 2.0))).astype(np.float32)
        out.append(d)
    return [out[0]] + [out[1 + (i % (len(out) - 1))] for i in range(n - 1)] if n > 1 else out


def timed(fn, sync, window):
    """ms per call of fn over a window of at least `window` seconds (warm call first)."""
    fn()
    sync()
    n = 1
    while True:
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        dt = time.perf_counter() - t0
        if dt >= window:
            return 1e3 * dt / n, n
        n = max(n + 1, int(n * min(10.0, 1.2 * window / max(dt, 1e-6))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='c2,c4')
    ap.add_argument('--members', default='1,8,32')
    ap.add_argument('--m-b', type=int, default=8)
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--only-b', action='store_true', help='part B alone (a commit without ensembles)')
    ap.add_argument('--trace', action='store_true', help='a few untimed sweeps of each kind, for rocprofv3 --kernel-trace')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('ensemble_profile: needs a GPU')
    import bench
    from cosmo_pol_amd import RadarOperator
    az, el = np.arange(360.0), np.full(360, 1.0)
    m_list = sorted({int(x) for x in args.members.split(',')} | {args.m_b})
    result = {'device': torch.cuda.get_device_name(0), 'window_s': args.window, 'workloads': {}}
    for wl in args.workloads.split(','):
        conf, hyds, cube, luts = bench.make_inputs(wl)
        n_gates = None
        rec = {'A': {}, 'B': {}}
        result['workloads'][wl] = rec

        def new_op():
            return RadarOperator(config=conf, luts=luts, output_variables='only_radar', lanes=1)

        def outputs(op, m):
            ng = len(op.constants.RANGE_RADAR)
            t = {k: torch.empty((m, 360, ng), dtype=torch.float32, device='cuda') for k in FIELDS}
            return t, {k: v.data_ptr() for k, v in t.items()}
        # ---- B: separate operators ----
        free_before = torch.cuda.mem_get_info()[0]
        ops_b = []
        for k, data in enumerate(member_cubes(cube, args.m_b)):
            op = new_op()
            op.load_model_arrays(data, cube['zlevels'], cube['proj_info'], cube['resolution'])
            ops_b.append((op,) + outputs(op, 1))
            op.simulate_rays(az, el, device_outputs=ops_b[-1][2])
            op.wait()
            if k == 0:
                per_op = free_before - torch.cuda.mem_get_info()[0]
        total = torch.cuda.mem_get_info()[1]
        rec['B']['resident_bytes_per_operator'] = int(per_op)
        rec['B']['operators_that_fit'] = int(total // max(per_op, 1))

        def run_b():
            for op, _, ptrs in ops_b:
                op.simulate_rays(az, el, device_outputs=ptrs)

        def sync_b():
            for op, _, _ in ops_b:
                op.wait()
        # ---- A: one operator, members beside the model ----
        op_a = None
        if not args.only_b:
            op_a = new_op()
            free0 = op_a._ctx.mem_info()[0]
            op_a.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
            op_a.simulate_rays(az, el, device_outputs=outputs(op_a, 1)[1])
            op_a.wait()
            free1 = torch.cuda.mem_get_info()[0]
            m_max = max(m_list)
            op_a.load_model_ensemble(member_cubes(cube, m_max), cube['zlevels'], cube['proj_info'], cube['resolution'])
            free2 = torch.cuda.mem_get_info()[0]
            rec['A']['resident_bytes_per_member'] = int((free1 - free2) // max(m_max - 1, 1))
            rec['A']['resident_bytes_first_member_with_tables'] = int(free0 - free1)
            rec['A']['members_that_fit'] = int(1 + (total - (free0 - free1)) // max(rec['A']['resident_bytes_per_member'], 1))
            keep = {m: outputs(op_a, m) for m in m_list}
        if args.trace:
            for _ in range(3):
                run_b()
                sync_b()
                if op_a is not None:
                    for form in ('shared', 'per_member'):
                        op_a.simulate_rays_ensemble(az, el, members=list(range(args.m_b)), form=form, device_outputs=keep[args.m_b][1])
                        op_a.wait()
        else:
            for rep in range(args.repeat):
                ms, n = timed(run_b, sync_b, args.window)
                rec['B'].setdefault('ms_per_member_sweep', []).append(ms / args.m_b)
                print('%s rep %d  B  M=%d: %.4f ms per member-sweep (%d rounds)' % (wl, rep, args.m_b, ms / args.m_b, n), flush=True)
                if op_a is None:
                    continue
                for m in m_list:
                    for form in (('shared', 'per_member') if m == args.m_b else ('shared',)):
                        def run_a(m=m, form=form):
                            op_a.simulate_rays_ensemble(az, el, members=list(range(m)), form=form, device_outputs=keep[m][1])
                        ms, n = timed(run_a, op_a.wait, args.window)
                        rec['A'].setdefault('%s_M%d_ms_per_member_sweep' % (form, m), []).append(ms / m)
                        print('%s rep %d  A  %s M=%d: %.4f ms per member-sweep (%d rounds)' % (wl, rep, form, m, ms / m, n), flush=True)
                if rep == 0:
                    rec['A']['launch_forms_shared'] = {k: int(v) for k, v in op_a._ctx.launch_forms().items()}
        for op, _, _ in ops_b:
            op.close()
        if op_a is not None:
            op_a.close()
        del ops_b, op_a
        torch.cuda.empty_cache()
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if args.out and not args.trace:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
