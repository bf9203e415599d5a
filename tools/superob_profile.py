#!/usr/bin/env python
"""Superobservations against the per-gate hand-over they replace.

Seeded inputs from bench.make_inputs('c2'); needs a GPU.  One process, the step bench.py reports as `value_host_outputs`: the
360 x 500 sweep at 8 elevations in turn over three lanes, page-locked outputs, pinned calls, one wait per window.

  A   today's full per-gate hand-over (9 observables, RVEL, the float64 mask: 52 B per gate over PCIe);
  B   superobservations 4 x 8 alone (simulate_rays_superob(..., Superob(4, 8)): 9 float32 means, RVEL, 10 uint16 counts per
      window, no per-gate array copied).

A and B alternate and the pair is repeated --repeat times (medians and spread); every window is at least --window seconds,
closed by waiting for every lane.  The same pair for an ensemble call of three members (the cube and two seeded perturbations,
form 'shared').  k_superob's own time comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/superob_profile.py --trace` (a few untimed sweeps of each kind); pass its
figure with --kernel-us to have it written into the JSON.  --only-a: A alone (a commit without the feature: the control).

NOT measured: other windows than 4 x 8, sub-beam volumes, more or fewer lanes in flight for the ensemble form.

  python tools/superob_profile.py --out profiles/superob_profile.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
N_LANES, N_CYCLE = 3, 8


def main():
    from ensemble_profile import timed
    from timed_profile import perturbed
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--rays', type=int, default=4)
    ap.add_argument('--gates', type=int, default=8)
    ap.add_argument('--small', action='store_true', help='the small test cube and tables instead of the bench grid')
    ap.add_argument('--only-a', action='store_true', help='the per-gate hand-over alone (runs on a commit without superobservations)')
    ap.add_argument('--trace', action='store_true', help='a few untimed sweeps of each kind, for rocprofv3 --kernel-trace')
    ap.add_argument('--kernel-us', type=float, default=None, help="k_superob's average from the rocprofv3 run (single sweep)")
    ap.add_argument('--kernel-us-ensemble', type=float, default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('superob_profile: needs a GPU')
    import bench
    from cosmo_pol_amd import RadarOperator
    conf, hyds, cube, luts = bench.make_inputs('c2', small=args.small)
    n_rays = 360
    az = np.arange(float(n_rays))
    els = [np.full(n_rays, 1.0 + 0.05 * k) for k in range(N_CYCLE)]
    grid = (cube['zlevels'], cube['proj_info'], cube['resolution'])
    states = [cube['data'], perturbed(cube['data'], 101), perturbed(cube['data'], 202)]
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar', lanes=N_LANES)
    op.load_model_ensemble(states, *grid)
    ng = len(op.constants.RANGE_RADAR)
    spec = None
    if not args.only_a:
        from cosmo_pol_amd import superob as SO
        spec = SO.Superob(args.rays, args.gates)
        cells = int(np.prod(SO.shape(n_rays, ng, spec)))
    gate_bytes = n_rays * ng * (9 * 4 + 8 + 8)              # 9 observables, RVEL, the float64 mask
    result = {'device': torch.cuda.get_device_name(0), 'window_s': args.window, 'n_rays': n_rays, 'n_gates': ng,
              'lanes': N_LANES, 'elevations': N_CYCLE, 'cube': 'small test cube' if args.small else 'bench grid',
              'not_measured': 'other windows, sub-beam volumes, other numbers of lanes in flight for the ensemble form'}
    if spec is not None:
        result['window'] = [spec.rays, spec.gates]
        result['min_valid_fraction'] = spec.min_valid_fraction
    counter = [0]

    def wait_all():
        for i in range(N_LANES):
            op.wait(i)

    def call(fn):
        def run():
            k = counter[0]
            counter[0] += 1
            return fn(az, els[k % N_CYCLE], pinned=True, lane=k % N_LANES)
        return run
    members = 3
    # kind: (A, B, rows per ray)
    kinds = {'sweep': (op.simulate_rays, lambda a, e, **kw: op.simulate_rays_superob(a, e, spec, **kw), 1),
             'ensemble': (lambda a, e, **kw: op.simulate_rays_ensemble(a, e, form='shared', **kw),
                          lambda a, e, **kw: op.simulate_rays_ensemble(a, e, form='shared', superob=spec, **kw), members)}
    for kind, (fn_a, fn_b, rows) in kinds.items():
        run_a = call(fn_a)
        run_b = call(fn_b) if spec is not None else None
        for _ in range(4 * N_CYCLE):                        # every table set, gate coordinate and stencil in place
            run_a()
            if run_b:
                run_b()
        wait_all()
        if args.trace:
            continue
        rec = {'A_ms': [], 'B_ms': [], 'A_pcie_bytes_per_call': gate_bytes * rows}
        result[kind] = rec
        if spec is not None:
            rec['B_pcie_bytes_per_call'] = cells * rows * (9 * 4 + 8 + 10 * 2)
            rec['bytes_A_over_B'] = rec['A_pcie_bytes_per_call'] / rec['B_pcie_bytes_per_call']
        for rep in range(args.repeat):
            for tag, run in (('A', run_a), ('B', run_b)):
                if run is None:
                    continue
                ms, n = timed(run, wait_all, args.window)
                rec[tag + '_ms'].append(ms)
                print('%s rep %d  %s: %.4f ms per call (%d calls)' % (kind, rep, tag, ms, n), flush=True)
        for tag in ('A', 'B'):
            v = rec[tag + '_ms']
            if v:
                rec[tag + '_ms_median'] = float(np.median(v))
                rec[tag + '_spread'] = float((max(v) - min(v)) / np.median(v))
        if rec['B_ms']:
            rec['B_over_A'] = rec['B_ms_median'] / rec['A_ms_median']
            rec['launch_forms_B'] = {k: int(v) for k, v in op._ctx.launch_forms().items()}
    if args.kernel_us is not None and 'sweep' in result:
        result['sweep']['k_superob_us'] = args.kernel_us
    if args.kernel_us_ensemble is not None and 'ensemble' in result:
        result['ensemble']['k_superob_us'] = args.kernel_us_ensemble
    op.close()
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if args.out and not args.trace:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
