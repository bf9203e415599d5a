#!/usr/bin/env python
"""tools/fractions_profile.py -- the fractions skill score on the device against the maps pulled to the host.

Seeded inputs from bench.make_inputs('c2'): the 360 x 500 bench sweep, one lane, an ensemble of --members states (the cube and
seeded perturbations, form 'shared'); per-member ZH 'max' maps on the 300 x 300 grid of 1 km cells, scored at three thresholds
(18, 30, 40 dBZ) and six radii (0, 1, 2, 5, 10, 20 cells) against the map of member 1.  Wall time per call around BLOCKING calls
with page-locked outputs (each ends in a device synchronise), in fresh processes that alternate:

  ens_fss    simulate_rays_ensemble_composite_fss: the maps and the scores from the device;
  ens_maps   simulate_rays_ensemble_composite: the same call without scores;
  ens_host   ens_maps, then neighbourhood.sums on the host: what the device call replaces;
  comp / parent_comp     simulate_rays_composite (no struct) of this tree and of --parent-tree DIR (a checkout of the parent commit
             with its library built): the control for "a call without the struct did not get slower";
  bench / parent_bench   (--bench) `python bench.py --gpus 1 --steps 20 --warmup 5` of this tree and of DIR: the result line.

Kernel times come from a run of its own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/fractions_profile.py --worker ens_fss --trace
pass the kernel statistics file with --kernel-stats NAME=FILE to have the figures of k_frac_rows, k_frac_cols and k_frac_score
written into the JSON.

With --probabilities the session measures the neighbourhood ensemble probabilities on the same workload and
writes profiles/fraction_probabilities_profile.json:

  ens_prob        ens_fss with a neighbourhood.Probabilities: the sums of the ensemble FSS and the reliability table too;
  ens_prob_maps   the same with the S and the A maps (maps=True, any_maps=True);
  ens_prob_host   ens_maps, then neighbourhood.ensemble_sums on the host: what the device call replaces;
  ens_fss / parent_ens_fss   the call with the Fractions alone of this tree and of --parent-tree DIR: the control for "a call
                  without the struct did not get slower" (with --bench: bench / parent_bench too);
each record carries the bytes handed over (every array of res['composite']); k_frac_members comes from --kernel-stats.

NOT measured: several lanes in flight, device-resident outputs, a domain mask, other grids, radii and member counts, the
single sweep's score, a volume's score.

  python tools/fractions_profile.py --repeat 3 --out profiles/fractions_profile.json
  python tools/fractions_profile.py --worker ens_fss            (one process, one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from composite_profile import inside, kernel_table, last_json_line  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = 360
THRESHOLDS_DBZ = [18.0, 30.0, 40.0]
RADII = [0, 1, 2, 5, 10, 20]
WORKERS = ('ens_fss', 'ens_maps', 'ens_host', 'comp', 'ens_prob', 'ens_prob_maps', 'ens_prob_host')
KERNELS = ('k_frac_rows', 'k_frac_cols', 'k_frac_score', 'k_frac_members', 'k_comp_combined', 'k_comp_finish')


def handed_over(w):
    """The bytes of every array under a result's 'composite' entry."""
    if isinstance(w, dict):
        return sum(handed_over(v) for v in w.values())
    return int(w.nbytes) if isinstance(w, np.ndarray) else 0


def worker(a):
    tree = os.path.abspath(a.tree)
    for p in (tree, os.path.join(tree, 'tools')):
        sys.path.insert(0, p)
    import bench
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_amd import composite as CP
    conf, hyds, cube, luts = bench.make_inputs('c2')
    az, el = np.arange(float(N_RAYS)), np.full(N_RAYS, 1.0)
    grid = (cube['zlevels'], cube['proj_info'], cube['resolution'])
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    e = CP.grid(150e3, 1e3)
    cspec = CP.Composite('ZH', e, e)
    if a.worker == 'comp':
        op.load_model_arrays(cube['data'], *grid)
        run = lambda: op.simulate_rays_composite(az, el, cspec)
    else:
        from timed_profile import perturbed
        from cosmo_pol_amd import neighbourhood as NB
        op.load_model_ensemble([cube['data']] + [perturbed(cube['data'], 100 + m) for m in range(1, a.members)], *grid)
        spec = NB.Fractions(cspec, 'ZH', CP.from_db(THRESHOLDS_DBZ), RADII)
        # the observed map: member 1's own (another state of the same model), made once, outside the timed calls
        observed = np.array(op.simulate_rays_ensemble_composite(az, el, cspec, members=[1])['composite']['values']['ZH']['max'][0])
        if a.worker == 'ens_fss':
            run = lambda: op.simulate_rays_ensemble_composite_fss(az, el, spec, observed)
        elif a.worker == 'ens_maps':
            run = lambda: op.simulate_rays_ensemble_composite(az, el, cspec)
        elif a.worker in ('ens_prob', 'ens_prob_maps'):
            pspec = NB.Probabilities(spec, maps=a.worker == 'ens_prob_maps', any_maps=a.worker == 'ens_prob_maps')
            run = lambda: op.simulate_rays_ensemble_composite_fss(az, el, pspec, observed)
        elif a.worker == 'ens_prob_host':
            def run():
                res = op.simulate_rays_ensemble_composite(az, el, cspec)
                res['composite']['probabilities'] = NB.ensemble_sums(spec, res['composite']['values']['ZH']['max'], observed)
                return res
        else:
            def run():
                res = op.simulate_rays_ensemble_composite(az, el, cspec)
                res['composite']['fractions'] = NB.sums(spec, res['composite']['values']['ZH']['max'], observed)
                return res
    if a.worker in ('ens_host', 'ens_prob_host'):            # (seconds per call: the rule holds int64 [members, 3, 6, 300, 300] several times over)
        a.warmup, a.steps = min(a.warmup, 1), min(a.steps, 3)
    for _ in range(a.warmup):
        res = run()
    if a.trace:
        op.close()
        return
    t = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        res = run()
        t.append((time.perf_counter() - t0) * 1e3)
    w = res['composite']
    out = {'call': a.worker, 'n_rays': N_RAYS, 'n_gates': len(op.constants.RANGE_RADAR), 'steps': a.steps,
           'ms_per_call_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
           'max_checksum': float(np.nansum(w['values']['ZH']['max'], dtype=np.float64)), 'counted': int(w['count']['ZH'].sum())}
    if a.worker != 'ens_prob_host':       # (the rule always makes both maps: not what a call hands over)
        out['bytes_handed_over'] = handed_over(w)
    if 'probabilities' in w:
        pr = w['probabilities']
        from cosmo_pol_amd import neighbourhood as NB
        k_of = np.arange(pr['n_blocks'] + 1, dtype=np.uint64)[:, None] * np.array([1, 1000], np.uint64)
        out['prob_checksum'] = [int(np.array(pr[k]).sum(dtype=np.uint64)) for k in ('diff2', 'forecast2', 'observed2')] + [
            int((np.array(pr['reliability']) * k_of).sum(dtype=np.uint64))]
        out['ensemble_fss'] = [[None if np.isnan(x) else float(x) for x in row] for row in NB.fss(pr)]
        out['brier'] = [[None if np.isnan(x) else float(x) for x in row] for row in NB.brier(pr)]
        out['thresholds_dbz'], out['radii'] = THRESHOLDS_DBZ, RADII
    if a.worker != 'comp':
        out['members'] = a.members
    if 'fractions' in w:
        fr = w['fractions']
        out['sums_checksum'] = [int(np.array(fr[k]).sum(dtype=np.uint64)) for k in ('diff2', 'forecast2', 'observed2')]
        from cosmo_pol_amd import neighbourhood as NB
        score = NB.fss(fr)
        out['fss_member_0'] = [[None if np.isnan(x) else float(x) for x in row] for row in score[0]]
        out['thresholds_dbz'], out['radii'] = THRESHOLDS_DBZ, RADII
    print(json.dumps(out))
    op.close()


def driver(a):
    here = os.path.abspath(__file__)
    tags = ['ens_fss', 'ens_maps', 'ens_host', 'comp']
    if a.probabilities:
        tags = ['ens_fss', 'ens_prob', 'ens_prob_maps', 'ens_prob_host']
    if a.parent_tree:
        tags.append('parent_ens_fss' if a.probabilities else 'parent_comp')
    if a.bench:
        tags += ['bench'] + (['parent_bench'] if a.parent_tree else [])
    if a.calls:
        tags = [t for t in a.calls.split(',') if t and t != 'none']       # (none: only --kernel-stats, with --update)
    runs = {t: [] for t in tags}
    common = ['--steps', str(a.steps), '--warmup', str(a.warmup), '--members', str(a.members)]
    for rep in range(a.repeat):
        for tag in tags:
            tree = os.path.abspath(a.parent_tree) if tag.startswith('parent_') else ROOT
            if tag.endswith('bench'):
                cmd = [sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5']
            else:
                cmd = [sys.executable, here, '--worker', tag.replace('parent_', ''), '--tree', tree] + common
            r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.process_timeout)
            if r.returncode != 0:
                raise SystemExit('fractions_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            if tag.endswith('bench'):
                print('rep %d  %-12s value %.4e gates/s, %.4f ms per step' % (rep, tag, rec['value'], rec['ms_per_step']), flush=True)
            else:
                print('rep %d  %-12s %.4f ms per call (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_call_median'], rec['ms_min'],
                                                                              rec['ms_max']), flush=True)
    result = {'workload': 'bench.make_inputs(c2): %d rays x 500 gates, one lane, %d members; per-member ZH max maps on 300 x 300 cells of '
                          '1 km, thresholds %s dBZ, radii %s cells, observed = the map of member 1' % (N_RAYS, a.members, THRESHOLDS_DBZ, RADII),
              'method': 'blocking calls with page-locked outputs, %d steps after %d warm-up calls per process, %d fresh processes per '
                        'call, alternating' % (a.steps, a.warmup, a.repeat),
              'not_measured': 'several lanes in flight, device-resident outputs, a domain mask, other grids, radii and member counts, '
                              "the single sweep's score, a volume's score",
              'calls': {}}
    for tag, recs in runs.items():
        if tag.endswith('bench'):
            v = [r['value'] for r in recs]
            result['calls'][tag] = {'value_median': float(np.median(v)), 'values': v, 'ms_per_step': [r['ms_per_step'] for r in recs],
                                    'spread': float((max(v) - min(v)) / np.median(v))}
            continue
        med = [r['ms_per_call_median'] for r in recs]
        c = {'ms_per_call_median_of_processes': float(np.median(med)), 'ms_per_call_medians': med,
             'spread': float((max(med) - min(med)) / np.median(med))}
        for k in ('max_checksum', 'counted', 'members', 'sums_checksum', 'fss_member_0', 'thresholds_dbz', 'radii', 'bytes_handed_over',
                  'prob_checksum', 'ensemble_fss', 'brier'):
            if k in recs[0]:
                c[k] = recs[0][k]
        result['calls'][tag] = c
    if a.update and a.out and os.path.exists(a.out):
        # a second session of the driver (another list of --calls): its calls and kernel tables join the file's
        with open(a.out) as f:
            old = json.load(f)
        old['calls'].update(result['calls'])
        old['method'] = result['method'] if old.get('method') == result['method'] else old.get('method', '') + '; ' + result['method']
        result = old
    calls = result['calls']
    ms = lambda tag: calls[tag]['ms_per_call_median_of_processes']       # noqa: E731
    if all(t in calls for t in ('ens_fss', 'ens_maps', 'ens_host')):
        result['scores_cost_ms'] = ms('ens_fss') - ms('ens_maps')
        result['host_scores_cost_ms'] = ms('ens_host') - ms('ens_maps')
        result['ens_fss_over_ens_host_ms'] = ms('ens_fss') / ms('ens_host')
        result['sums_equal'] = bool(calls['ens_fss'].get('sums_checksum') == calls['ens_host'].get('sums_checksum')
                                    and calls['ens_fss'].get('max_checksum') == calls['ens_host'].get('max_checksum'))
    if all(t in calls for t in ('ens_fss', 'ens_prob', 'ens_prob_maps', 'ens_prob_host')):
        result['probabilities_cost_ms'] = ms('ens_prob') - ms('ens_fss')
        result['probabilities_with_maps_cost_ms'] = ms('ens_prob_maps') - ms('ens_fss')
        result['ens_prob_over_ens_prob_host_ms'] = ms('ens_prob') / ms('ens_prob_host')
        result['prob_sums_equal'] = bool(calls['ens_prob'].get('prob_checksum') == calls['ens_prob_host'].get('prob_checksum')
                                         == calls['ens_prob_maps'].get('prob_checksum')
                                         and calls['ens_prob'].get('max_checksum') == calls['ens_prob_host'].get('max_checksum'))
    if 'parent_ens_fss' in calls and 'ens_fss' in calls:
        cc, pc = calls['ens_fss'], calls['parent_ens_fss']
        result['control_fractions'] = {'ens_fss_over_parent_ens_fss_ms': ms('ens_fss') / ms('parent_ens_fss'),
                                       'range_ms': [min(cc['ms_per_call_medians']), max(cc['ms_per_call_medians'])],
                                       'parent_range_ms': [min(pc['ms_per_call_medians']), max(pc['ms_per_call_medians'])],
                                       'each_median_inside_the_others_range': inside(cc['ms_per_call_medians'], pc['ms_per_call_medians']),
                                       'checksum_equal': bool(pc.get('max_checksum') == cc.get('max_checksum')
                                                              and pc.get('sums_checksum') == cc.get('sums_checksum'))}
    if 'parent_comp' in calls and 'comp' in calls:
        cc, pc = calls['comp'], calls['parent_comp']
        result['control_composite'] = {'comp_over_parent_comp_ms': ms('comp') / ms('parent_comp'),
                                       'range_ms': [min(cc['ms_per_call_medians']), max(cc['ms_per_call_medians'])],
                                       'parent_range_ms': [min(pc['ms_per_call_medians']), max(pc['ms_per_call_medians'])],
                                       'each_median_inside_the_others_range': inside(cc['ms_per_call_medians'], pc['ms_per_call_medians']),
                                       'checksum_equal': bool(pc.get('max_checksum') == cc.get('max_checksum'))}
    if 'parent_bench' in calls and 'bench' in calls:
        b, pb = calls['bench'], calls['parent_bench']
        result['control_bench'] = {'value_over_parent': b['value_median'] / pb['value_median'],
                                   'range': [min(b['values']), max(b['values'])], 'parent_range': [min(pb['values']), max(pb['values'])],
                                   'each_median_inside_the_others_range': inside(b['values'], pb['values'])}
    for item in a.kernel_stats or []:
        name, path = item.split('=', 1)
        tb = kernel_table(path)
        # (the profiler's database names kernels as the code object does, _Z14k_frac_members12FracProbArgs.kd: found by the bare name)
        found = {k: tb.get(k) or next((v for n, v in sorted(tb.items()) if k in n), None) for k in KERNELS}
        result.setdefault('kernels', {})[name] = found
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', choices=WORKERS, default=None, help='one process of one call: prints one JSON line')
    ap.add_argument('--tree', default=ROOT, help='with --worker: the checkout whose package and bench inputs are used')
    ap.add_argument('--trace', action='store_true', help='with --worker: the warm-up calls alone, for rocprofv3 --kernel-trace')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--members', type=int, default=21, help='members of the ensemble')
    ap.add_argument('--repeat', type=int, default=3, help='fresh processes per call')
    ap.add_argument('--calls', default=None, help='the calls of this session of the driver, comma-separated (default: all that apply)')
    ap.add_argument('--update', action='store_true', help='join the calls of this session to those --out already holds')
    ap.add_argument('--probabilities', action='store_true',
                    help='the session of the neighbourhood ensemble probabilities (default --out: profiles/fraction_probabilities_profile.json)')
    ap.add_argument('--bench', action='store_true', help="bench.py's result line too (of the parent tree as well)")
    ap.add_argument('--process-timeout', type=float, default=400.0)
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--kernel-stats', action='append', default=None, metavar='NAME=FILE')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.probabilities and not a.out and not a.worker:
        a.out = os.path.join(ROOT, 'profiles', 'fraction_probabilities_profile.json')
    if a.worker:
        worker(a)
    else:
        driver(a)


if __name__ == '__main__':
    main()
