#!/usr/bin/env python
"""Ensemble statistics against the per-member hand-over they replace.

Seeded inputs from bench.make_inputs('c2'); needs a GPU.  One process, one lane, the 360 x 500 bench sweep, an ensemble of M
members (the cube and seeded perturbations of it, made the way tests/test_gpu_ensemble.py makes its members, without the
planted bad values), for M in --members (default 3 and 21) and both forms ('shared', 'per_member'):

  A   simulate_rays_ensemble with page-locked outputs (pinned=True, then wait): every member's per-gate arrays over PCIe;
  B   simulate_rays_ensemble_stats(..., EnsembleStats(exceed={'ZH': [dbz(20), dbz(35)]}), pinned=True), then wait: mean,
      spread and count of every field and two ZH thresholds -- no per-member array is copied.

  C   (--quantiles) B with the three ZH quantiles 0.1, 0.5, 0.9 (EnsembleQuantiles): k_member_fold stashes ZH's members,
      k_member_quantile sorts them per gate.  With it the host part of the slow way is timed too, separately (A_host_ms):
      np.nanquantile(ZH, [0.1, 0.5, 0.9], axis=0) on the members A handed over -- the claim to check is C < A + A_host, and
      C < A alone.

A and B (and C) alternate and the pair is repeated --repeat times (medians and spread); every window is at least --window seconds,
closed by waiting for the lane.  PCIe bytes are counted from the arrays of the results.  The kernels' own times come from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/member_stats_profile.py --trace` (a few untimed calls of
each kind); pass its kernel statistics file with --kernel-stats to have k_member_fold / k_member_finish / k_member_quantile
written into the JSON.
--only-members: A alone (runs on a commit without the feature: the control for "existing calls did not get slower").

NOT measured: sub-beam volumes, several lanes in flight, device-resident outputs, other sets of statistics.

  python tools/member_stats_profile.py --out profiles/member_stats_profile.json
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
GEOM = ('lats', 'lons', 'dist', 'heights')


def result_bytes(res):
    """bytes of the arrays a call copied to the host (the shared gate coordinates are copied once per table set: not counted)"""
    keys = list(res.keys())
    n = 0
    for k in keys:
        if k in GEOM or k == 'stats' or (k == 'mask' and 'mask_sum8' in keys):
            continue
        if isinstance(res[k], np.ndarray):
            n += res[k].nbytes
    if 'stats' in res:
        s = res['stats']
        cells = next(iter(s['count'].values())).size
        n += 10 * cells * 2                                 # the count block: ten rows, whatever is folded
        n += sum(a.nbytes for kind, v in s.items() if kind not in ('count', 'n_members') for a in v.values())
    return int(n)


def kernel_stats(path):
    """{kernel: {'calls', 'avg_us', 'min_us', 'max_us'}} of the k_member_* kernels from rocprofv3's kernel statistics"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name', '')
            for k in ('k_member_fold', 'k_member_finish', 'k_member_quantile'):
                if name.startswith(k):
                    out[k] = {'calls': int(row['Calls']), 'avg_us': float(row['AverageNs']) / 1e3,
                              'min_us': float(row['MinNs']) / 1e3, 'max_us': float(row['MaxNs']) / 1e3}
    return out


def main():
    from ensemble_profile import timed
    from timed_profile import perturbed
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', default='3,21')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--small', action='store_true', help='the small test cube and tables instead of the bench grid')
    ap.add_argument('--only-members', action='store_true', help='the per-member hand-over alone (runs on a commit without the feature)')
    ap.add_argument('--quantiles', action='store_true', help='C: the statistics call with three ZH quantiles; and the host part of A')
    ap.add_argument('--trace', action='store_true', help='a few untimed calls of each kind, for rocprofv3 --kernel-trace')
    ap.add_argument('--kernel-stats', default=None, help="rocprofv3's kernel statistics file of a --trace run")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('member_stats_profile: needs a GPU')
    import bench
    from cosmo_pol_amd import RadarOperator
    conf, hyds, cube, luts = bench.make_inputs('c2', small=args.small)
    n_rays = 360
    az, el = np.arange(float(n_rays)), np.full(n_rays, 1.0)
    m_list = sorted(int(x) for x in args.members.split(','))
    states = [cube['data']] + [perturbed(cube['data'], 100 + i) for i in range(1, max(m_list))]
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar', lanes=1)
    op.load_model_ensemble(states, cube['zlevels'], cube['proj_info'], cube['resolution'])
    ng = len(op.constants.RANGE_RADAR)
    spec = None
    if not args.only_members:
        from cosmo_pol_amd import ensemble_stats as ES
        spec = ES.EnsembleStats(exceed={'ZH': [ES.dbz(20.0), ES.dbz(35.0)]})
    qspec = None
    if args.quantiles and spec is not None:
        qspec = ES.EnsembleQuantiles({'ZH': [0.1, 0.5, 0.9]}, exceed={'ZH': [ES.dbz(20.0), ES.dbz(35.0)]})
    result = {'device': torch.cuda.get_device_name(0), 'window_s': args.window, 'n_rays': n_rays, 'n_gates': ng, 'lanes': 1,
              'cube': 'small test cube' if args.small else 'bench grid', 'calls': {},
              'not_measured': 'sub-beam volumes, several lanes in flight, device-resident outputs, other sets of statistics'}
    if spec is not None:
        result['statistics'] = repr(spec)
    if qspec is not None:
        result['statistics_C'] = repr(qspec)
    for m in m_list:
        members = list(range(m))
        for form in ('shared', 'per_member'):
            def run_a():
                return op.simulate_rays_ensemble(az, el, members=members, form=form, pinned=True)

            def run_b():
                return op.simulate_rays_ensemble_stats(az, el, spec, members=members, form=form, pinned=True)

            def run_c():
                return op.simulate_rays_ensemble_stats(az, el, qspec, members=members, form=form, pinned=True)
            rc = None
            for _ in range(4):                              # every table set, gate coordinate and stencil in place
                ra = run_a()
                rb = run_b() if spec is not None else None
                rc = run_c() if qspec is not None else None
            op.wait()
            if args.trace:
                continue
            rec = {'A_ms': [], 'B_ms': [], 'A_pcie_bytes_per_call': result_bytes(ra)}
            result['calls']['M%d_%s' % (m, form)] = rec
            if rb is not None:
                rec['B_pcie_bytes_per_call'] = result_bytes(rb)
                rec['bytes_A_over_B'] = rec['A_pcie_bytes_per_call'] / rec['B_pcie_bytes_per_call']
                rec['launch_forms_B'] = {k: int(v) for k, v in op._ctx.launch_forms().items()}
            if rc is not None:
                import time
                import warnings
                rec['C_ms'] = []
                rec['C_pcie_bytes_per_call'] = result_bytes(rc)
                rec['bytes_A_over_C'] = rec['A_pcie_bytes_per_call'] / rec['C_pcie_bytes_per_call']
                host = []
                for _ in range(args.repeat):               # the host part of the slow way, on the members A handed over
                    t0 = time.perf_counter()
                    with warnings.catch_warnings():
                        warnings.simplefilter('ignore')
                        ref = np.nanquantile(ra['ZH'], [0.1, 0.5, 0.9], axis=0)
                    host.append((time.perf_counter() - t0) * 1e3)
                rec['A_host_ms'] = host
                rec['A_host_ms_median'] = float(np.median(host))
                got = rc['stats']['quantile']['ZH']
                rec['C_max_rel_dev_from_nanquantile'] = float(np.nanmax(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300), initial=0.0))
                del ref, got
            del ra, rb, rc
            for rep in range(args.repeat):
                for tag, run in (('A', run_a), ('B', run_b if spec is not None else None), ('C', run_c if qspec is not None else None)):
                    if run is None:
                        continue
                    ms, n = timed(run, op.wait, args.window)
                    rec[tag + '_ms'].append(ms)
                    print('M=%d %s rep %d  %s: %.4f ms per call (%d calls)' % (m, form, rep, tag, ms, n), flush=True)
            for tag in ('A', 'B', 'C'):
                v = rec.get(tag + '_ms')
                if v:
                    rec[tag + '_ms_median'] = float(np.median(v))
                    rec[tag + '_spread'] = float((max(v) - min(v)) / np.median(v))
            if rec['B_ms']:
                rec['B_over_A'] = rec['B_ms_median'] / rec['A_ms_median']
            if rec.get('C_ms'):
                rec['C_over_A'] = rec['C_ms_median'] / rec['A_ms_median']
                rec['C_over_B'] = rec['C_ms_median'] / rec['B_ms_median']
                rec['C_below_A'] = bool(rec['C_ms_median'] < rec['A_ms_median'])
    if args.kernel_stats:
        result['kernels'] = kernel_stats(args.kernel_stats)
    op.close()
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if args.out and not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
