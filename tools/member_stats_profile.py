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

--verify: the VERIFICATION of the ensemble against an observed sweep, M = 21, the operator's own form, in
fresh processes that alternate:
  V   simulate_rays_ensemble_verify(..., EnsembleVerification(verify=['ZH'], exceed=B's)), B's statistics plus the ranks and the
      CRPS of ZH against an observed sweep (member 0's ZH times 1.3, every seventh gate without an observation);
  B   the statistics call of above without the verification, in the same process as V;
  A   the per-member hand-over, and separately the host part of the slow way on the members it handed over
      (ensemble_verify.verify: A_host_ms);
  B on this tree and B on --parent-tree DIR (a checkout of the parent commit with its library built), each measured by the
  tree's own default mode of this tool, --repeat processes of each, alternating: the condition is that the statistics call
  without the struct lies inside the parent's run-to-run spread.
k_member_verify's own time comes from rocprofv3's kernel statistics of a `--verify-worker --trace` run (--kernel-stats).

  python tools/member_stats_profile.py --verify --parent-tree DIR --out profiles/member_verify_profile.json
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

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
        n += sum(a.nbytes for kind, v in s.items() if kind not in ('count', 'n_members', 'verify') for a in v.values())
        n += sum(a.nbytes for v in s.get('verify', {}).values() for a in v.values())
    return int(n)


def kernel_stats(path):
    """{kernel: {'calls', 'avg_us', 'min_us', 'max_us'}} of the k_member_* kernels from rocprofv3's kernel statistics"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name', '')
            for k in ('k_member_fold', 'k_member_finish', 'k_member_quantile', 'k_member_verify'):
                if name.startswith(k):
                    out[k] = {'calls': int(row['Calls']), 'avg_us': float(row['AverageNs']) / 1e3,
                              'min_us': float(row['MinNs']) / 1e3, 'max_us': float(row['MaxNs']) / 1e3}
    return out


def verify_worker(args):
    """One process of --verify: V, B and A on the 21-member sweep, alternating windows; one JSON line."""
    from ensemble_profile import timed
    from timed_profile import perturbed
    import bench
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_amd import ensemble_stats as ES
    from cosmo_pol_amd import ensemble_verify as EV
    conf, hyds, cube, luts = bench.make_inputs('c2', small=args.small)
    n_rays, m = 360, 21
    az, el = np.arange(float(n_rays)), np.full(n_rays, 1.0)
    states = [cube['data']] + [perturbed(cube['data'], 100 + i) for i in range(1, m)]
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar', lanes=1)
    op.load_model_ensemble(states, cube['zlevels'], cube['proj_info'], cube['resolution'])
    exceed = {'ZH': [ES.dbz(20.0), ES.dbz(35.0)]}
    spec, vspec = ES.EnsembleStats(exceed=exceed), EV.EnsembleVerification(verify=['ZH'], exceed=exceed)
    ra = op.simulate_rays_ensemble(az, el)
    y = (np.array(ra['ZH'][0]) * np.float32(1.3)).astype(np.float32)
    y.reshape(-1)[::7] = np.nan
    obs = {'ZH': y}

    def run_v():
        return op.simulate_rays_ensemble_verify(az, el, vspec, obs, pinned=True)

    def run_b():
        return op.simulate_rays_ensemble_stats(az, el, spec, pinned=True)

    def run_a():
        return op.simulate_rays_ensemble(az, el, pinned=True)
    for _ in range(4):                                      # every table set, gate coordinate and stencil in place
        ra, rb, rv = run_a(), run_b(), run_v()
    op.wait()
    if args.trace:
        op.close()
        return
    rec = {'n_rays': n_rays, 'n_gates': int(y.shape[1]), 'members': m, 'V_ms': [], 'B_ms': [], 'A_ms': [], 'A_host_ms': [],
           'V_bytes_handed_over': result_bytes(rv), 'V_observation_bytes_to_device': int(y.nbytes), 'B_bytes_handed_over': result_bytes(rb),
           'A_bytes_handed_over': result_bytes(ra), 'launch_forms_V': {k: int(v) for k, v in op._ctx.launch_forms().items()},
           'statistics_V': repr(vspec), 'statistics_B': repr(spec)}
    members = np.array(ra['ZH'])
    for _ in range(args.repeat):                            # the host part of the slow way, on the members A handed over
        t0 = time.perf_counter()
        ref = EV.verify(members, y)
        rec['A_host_ms'].append((time.perf_counter() - t0) * 1e3)
    got = rv['stats']['verify']
    rec['V_equals_host_rule'] = bool(all(np.array_equal(got[k]['ZH'], ref[k], equal_nan=k == 'crps') for k in EV.OUTPUTS))
    rec['crps_nanmean'] = float(np.nanmean(ref['crps']))
    del ra, rb, rv, members, got, ref
    for rep in range(args.repeat):
        for tag, run in (('V', run_v), ('B', run_b), ('A', run_a)):
            ms, n = timed(run, op.wait, args.window)
            rec[tag + '_ms'].append(ms)
            print('rep %d  %s: %.4f ms per call (%d calls)' % (rep, tag, ms, n), flush=True)
    op.close()
    print(json.dumps(rec))


def last_json_line(text):
    """the last JSON object of a process's output: the worker's one line, or the default mode's indented result"""
    text = '\n' + text
    at = len(text)
    while True:
        at = text.rindex('\n{', 0, at)
        try:
            return json.JSONDecoder().raw_decode(text[at + 1:])[0]
        except ValueError:
            continue


def verify_driver(args):
    """--verify: the worker and the default mode of this tree and of the parent's, in fresh processes, alternating."""
    here = os.path.abspath(__file__)
    common = ['--repeat', '1', '--window', str(args.window)] + (['--small'] if args.small else [])
    plans = [('worker', [sys.executable, here, '--verify-worker'] + common, ROOT),
             ('branch', [sys.executable, here, '--members', '21'] + common, ROOT)]
    if args.parent_tree:
        tree = os.path.abspath(args.parent_tree)
        plans.append(('parent', [sys.executable, os.path.join(tree, 'tools', 'member_stats_profile.py'), '--members', '21'] + common, tree))
    runs = {tag: [] for tag, _, _ in plans}
    for rep in range(args.repeat):
        for tag, cmd, cwd in plans:
            r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.process_timeout)
            if r.returncode != 0:
                raise SystemExit('member_stats_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            shown = rec['V_ms'] if tag == 'worker' else rec['calls']['M21_shared']['B_ms']
            print('rep %d  %-7s %s' % (rep, tag, ['%.4f' % v for v in shown]), flush=True)
    w = runs['worker']
    result = {'workload': '21 members, %d rays x %d gates, one lane, page-locked outputs' % (w[0]['n_rays'], w[0]['n_gates']),
              'method': 'windows of at least %.2f s closed by waiting for the lane; %d fresh processes of each kind, alternating'
                        % (args.window, args.repeat),
              'not_measured': 'sub-beam volumes, several lanes in flight, device-resident observations and outputs, more than one '
                              'verified field, RVEL (float64 keys), ensembles of other sizes',
              'calls': {}}
    for k in ('statistics_V', 'statistics_B', 'launch_forms_V', 'V_equals_host_rule', 'crps_nanmean', 'V_bytes_handed_over',
              'V_observation_bytes_to_device', 'B_bytes_handed_over', 'A_bytes_handed_over'):
        result[k] = w[0][k]
    for tag in ('V', 'B', 'A', 'A_host'):
        v = [x for r in w for x in r[tag + '_ms']]
        result['calls'][tag] = {'ms': v, 'ms_median': float(np.median(v)), 'spread': float((max(v) - min(v)) / np.median(v))}
    c = result['calls']
    result['V_minus_B_ms'] = c['V']['ms_median'] - c['B']['ms_median']
    result['V_over_A_plus_host'] = c['V']['ms_median'] / (c['A']['ms_median'] + c['A_host']['ms_median'])
    result['bytes_A_over_V'] = result['A_bytes_handed_over'] / (result['V_bytes_handed_over'] + result['V_observation_bytes_to_device'])
    for form in ('shared', 'per_member'):
        b = [x for r in runs['branch'] for x in r['calls']['M21_' + form]['B_ms']]
        c['B_default_mode_' + form] = {'ms': b, 'ms_median': float(np.median(b))}
        if 'parent' in runs:
            p = [x for r in runs['parent'] for x in r['calls']['M21_' + form]['B_ms']]
            c['B_parent_' + form] = {'ms': p, 'ms_median': float(np.median(p))}
            result['B_over_parent_' + form] = float(np.median(b) / np.median(p))
            # inside the run-to-run spread of the two: the median of either lies inside the range the other's processes span
            result['B_inside_spread_of_parent_' + form] = bool(min(p) <= np.median(b) <= max(p) or min(b) <= np.median(p) <= max(b))
    if 'parent' not in runs:
        result['not_measured'] += '; the parent commit (no --parent-tree)'
    if args.kernel_stats:
        result['kernels'] = kernel_stats(args.kernel_stats)
    else:
        result['not_measured'] += "; the kernels' own times (no --kernel-stats)"
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


def main():
    from ensemble_profile import timed
    from timed_profile import perturbed
    ap = argparse.ArgumentParser()
    ap.add_argument('--verify', action='store_true', help='the verification against an observed sweep, with the parent commit as the control')
    ap.add_argument('--verify-worker', action='store_true', help='one process of --verify')
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--process-timeout', type=float, default=400.0)
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
    if args.verify:
        return verify_driver(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('member_stats_profile: needs a GPU')
    if args.verify_worker:
        return verify_worker(args)
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
