#!/usr/bin/env python
"""Time-interpolated sweeps against the ensemble sweep they share their gathers with, and against what a user does without
them.

Seeded inputs from bench.make_inputs; needs a GPU.  Two shapes, device-resident outputs: the bench C2 sweep (360 x 500 gates, one
sub-beam) and the 225-ray share of the C4 volume (225 x 500, 7 x 7 sub-beams).  Three states of the bench cube are staged as a
series (the cube and two seeded perturbations of it; --small: the small test cube).  Per shape:

  T   simulate_rays_at with every ray between states 0 and 1 at a weight > 0 (every gate gathers from both cubes), two sets of
      ray times in turn (every call uploads its per-ray brackets);
  M2  simulate_rays_ensemble(form='shared') over the same two states (the same gathers, twice the rows in the second half);
  H   what a user does without the mode, ONCE: timeline.blend_states on the host + load_model_arrays + simulate_rays.

T and M2 alternate in one process and the pair is repeated --repeat times (the spread); every window is at least --window
seconds of device work, closed by the context's synchronize.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/timed_profile.py --trace` (a few untimed sweeps of each kind).

  python tools/timed_profile.py --out profiles/timed_profile.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V']
SERIES = [0.0, 600.0, 1500.0]
SHAPES = {'c2': 360, 'c4': 225}


def perturbed(data, seed):
    """A seeded other state of the same model: hydrometeor masses scaled by 0.5 - 2 per variable, T 3 K colder."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in sorted(data):
        v = data[k]
        if k.startswith('Q') and k.endswith('_v'):
            out[k] = (v * np.float32(rng.uniform(0.5, 2.0))).astype(np.float32)
        elif k == 'T':
            out[k] = (v - np.float32(3.0)).astype(np.float32)
        else:
            out[k] = v
    return out


def main():
    from ensemble_profile import timed
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='c2,c4')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--small', action='store_true', help='the small test cube and tables instead of the bench grid')
    ap.add_argument('--trace', action='store_true', help='a few untimed sweeps of each kind, for rocprofv3 --kernel-trace')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('timed_profile: needs a GPU')
    import bench
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_amd import timeline
    result = {'device': torch.cuda.get_device_name(0), 'window_s': args.window, 'series_s': SERIES,
              'cube': 'small test cube' if args.small else 'bench grid', 'workloads': {}}
    for wl in args.workloads.split(','):
        print('%s: making the inputs ...' % wl, flush=True)
        conf, hyds, cube, luts = bench.make_inputs(wl, small=args.small)
        n_rays = SHAPES[wl]
        az, el = np.arange(float(n_rays)), np.full(n_rays, 1.0)
        states = [cube['data'], perturbed(cube['data'], 101), perturbed(cube['data'], 202)]
        grid = (cube['zlevels'], cube['proj_info'], cube['resolution'])
        rec = {'n_rays': n_rays, 'cube_shape': list(np.shape(cube['zlevels'])), 'T_ms': [], 'M2_ms': []}
        result['workloads'][wl] = rec
        op = RadarOperator(config=conf, luts=luts, output_variables='only_radar', lanes=1)
        op.load_model_series(states, SERIES, *grid)
        print('%s: three states staged' % wl, flush=True)
        ng = len(op.constants.RANGE_RADAR)
        rec['n_gates'], rec['n_vars'] = ng, len(op._staged_vars)
        rec['n_sub'] = None
        # every ray at its own weight in (0, 1): t between states 0 and 1
        # (two sets of times used in turn: every call brings brackets the device does not hold yet, as the sweeps of a real scan do)
        t_rays = [600.0 * (0.05 + 0.9 * (np.arange(n_rays) + 0.5) / n_rays), 600.0 * (0.95 - 0.9 * (np.arange(n_rays) + 0.5) / n_rays)]
        turn = [0]
        out_t = {k: torch.empty((n_rays, ng), dtype=torch.float32, device='cuda') for k in FIELDS}
        out_m = {k: torch.empty((2, n_rays, ng), dtype=torch.float32, device='cuda') for k in FIELDS}
        ptr_t = {k: v.data_ptr() for k, v in out_t.items()}
        ptr_m = {k: v.data_ptr() for k, v in out_m.items()}

        def run_t():
            turn[0] ^= 1
            op.simulate_rays_at(az, el, t_rays[turn[0]], device_outputs=ptr_t)

        def run_m2():
            op.simulate_rays_ensemble(az, el, members=[0, 1], form='shared', device_outputs=ptr_m)
        if args.trace:
            for _ in range(3):
                run_t()
                op.wait()
                run_m2()
                op.wait()
        else:
            for rep in range(args.repeat):
                for tag, fn in (('T', run_t), ('M2', run_m2)):
                    ms, n = timed(fn, op.wait, args.window)
                    rec[tag + '_ms'].append(ms)
                    if tag == 'T' and rep == 0:
                        rec['launch_forms_T'] = {k: int(v) for k, v in op._ctx.launch_forms().items()}
                        rec['n_sub'] = rec['launch_forms_T']['n_sub']
                    print('%s rep %d  %-2s: %.4f ms per call (%d rounds)' % (wl, rep, tag, ms, n), flush=True)
            rec['T_over_M2'] = float(np.median(rec['T_ms']) / np.median(rec['M2_ms']))
            rec['spread_T'] = float((max(rec['T_ms']) - min(rec['T_ms'])) / np.median(rec['T_ms']))
            rec['spread_M2'] = float((max(rec['M2_ms']) - min(rec['M2_ms'])) / np.median(rec['M2_ms']))
            # ---- H: the host blend, once ----
            w = np.float32(0.25)
            t0 = time.perf_counter()
            data = timeline.blend_states(states[0], states[1], w)
            t1 = time.perf_counter()
            op_h = RadarOperator(config=conf, luts=luts, output_variables='only_radar', lanes=1)
            t1b = time.perf_counter()
            op_h.load_model_arrays(data, *grid)
            op_h.wait()
            t2 = time.perf_counter()
            op_h.simulate_rays(az, el, device_outputs=ptr_t)
            op_h.wait()
            t3 = time.perf_counter()
            rec['H_s'] = {'blend_states': t1 - t0, 'load_model_arrays': t2 - t1b, 'first_simulate_rays': t3 - t2,
                          'total': (t1 - t0) + (t2 - t1b) + (t3 - t2)}
            print('%s H: blend %.3f s + load %.3f s + sweep %.3f s' % (wl, t1 - t0, t2 - t1b, t3 - t2), flush=True)
            # the same bits either way (every ray at w = 0.25)
            h_zh = out_t['ZH'].clone()
            op.simulate_rays_at(az, el, 150.0, device_outputs=ptr_t)
            op.wait()
            rec['T_equals_H_bitwise'] = bool(torch.equal(h_zh.view(torch.int32), out_t['ZH'].view(torch.int32)))
            op_h.close()
            del op_h, data
        op.close()
        del op, out_t, out_m
        torch.cuda.empty_cache()
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if args.out and not args.trace:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
