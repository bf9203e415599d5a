#!/usr/bin/env python
"""tools/spectrum_moments_profile.py -- the spectrum moments against the hand-over of the spectrum they replace.

Workload and method of tools/spectrum_broadening_profile.py: the `radial_d3_turb_fft256` configuration (tests/_broadening.py:
60 gates of 300 m, FFT_length 256 = 257 bins, one sub-beam, rain / snow / graupel / ice, turbulence broadening) widened to a PPI
of --rays azimuths; wall time per sweep around BLOCKING calls with page-locked outputs (each ends in a device synchronise), in
fresh processes that alternate:

  a   simulate_rays: the spectrum delivered (44 MB at 360 rays);
  b   simulate_rays_moments(..., all eight fields): the moments, no spectrum;
  c   simulate_rays_moments(..., keep_spectrum=True): both;
  parent_a   (--parent-tree DIR: a checkout of the parent commit with its library built) DIR's own
      tools/spectrum_broadening_profile.py --turb 1 --motion 0, which is call (a): the control for "existing calls did not get slower".

The bytes handed over are counted from the arrays of the results (the shared gate coordinates are copied once per table set: not
counted).  Kernel times come from runs of their own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/spectrum_moments_profile.py --worker b --trace
(a few untimed calls); pass the kernel statistics files with --kernel-stats-a / -b / -parent to have k_spec_moments, its share of
the scheme-3 kernel list and the comparison of (a)'s kernel list with the parent's written into the JSON.

NOT measured: sub-beam volumes, longer spectra, several lanes in flight, device-resident outputs, a partial field list.

  python tools/spectrum_moments_profile.py --repeat 5 --out profiles/spectrum_moments_profile.json
  python tools/spectrum_moments_profile.py --worker b            (one process, one JSON line)
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
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
GEOM = ('lats', 'lons', 'dist', 'heights')


def result_bytes(res):
    """bytes of the arrays a call copied to the host"""
    keys = list(res.keys())
    n = 0
    for k in keys:
        if k in GEOM or k == 'moments' or (k == 'mask' and 'mask_sum8' in keys):
            continue
        if isinstance(res[k], np.ndarray):
            n += res[k].nbytes
    if 'moments' in res:
        cells = res['moments']['count'].size
        n += 8 * cells * 8 + cells * 2                    # the block of eight rows, whatever is asked for, and the counts
    return int(n)


def worker(a):
    import _broadening as B
    import _cases
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_oracle import config as ocfg
    B.CASES['profile'] = ('d3_1mom_ice_sub', {'radar': {'FFT_length': 256}, 'integration': {'nh_GH': 1, 'nv_GH': 1},
                                              'doppler': {'turbulence_correction': 1, 'motion_correction': 0}}, None)
    over, az, el, cube, two = B.case_inputs('profile')
    conf = ocfg.make_config(over)
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme'])
            for h in ocfg.hydrometeor_list(conf)}
    op = RadarOperator(config=over, luts=luts, output_variables='only_radar')
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    azs, els = np.arange(a.rays) * (360.0 / a.rays), np.full(a.rays, el)
    if a.worker == 'a':
        run = lambda: op.simulate_rays(azs, els)
    else:
        from cosmo_pol_amd import spectrum_moments as SM
        spec = SM.SpectrumMoments(fields=SM.FIELDS)
        run = lambda: op.simulate_rays_moments(azs, els, spec, keep_spectrum=a.worker == 'c')
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
    out = {'call': a.worker, 'n_rays': a.rays, 'n_gates': int(res['ZH'].shape[1]), 'n_vbins': len(op.constants.VARRAY),
           'steps': a.steps, 'ms_per_sweep_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
           'bytes_handed_over': result_bytes(res)}
    if 'DSPECTRUM' in res:
        out['spectrum_checksum'] = float(np.nansum(res['DSPECTRUM']))
    if 'moments' in res:
        m = res['moments']
        out['width_nanmean'] = float(np.nanmean(m['WIDTH']))
        out['kurtosis_nanmedian'] = float(np.nanmedian(m['KURTOSIS']))
        out['gates_with_moments'] = int(np.isfinite(m['POWER']).sum())
    print(json.dumps(out))
    op.close()


def kernel_table(path):
    """{kernel: {'calls', 'total_us', 'avg_us', 'min_us', 'max_us'}} from rocprofv3's kernel statistics (names cut at the first
    bracket or parenthesis: template and argument lists away)"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name', '').split('(')[0].split('<')[0].strip()
            if not name:
                continue
            r = out.setdefault(name, {'calls': 0, 'total_us': 0.0, 'min_us': float('inf'), 'max_us': 0.0})
            r['calls'] += int(row['Calls'])
            r['total_us'] += float(row['TotalDurationNs']) / 1e3
            r['min_us'] = min(r['min_us'], float(row['MinNs']) / 1e3)
            r['max_us'] = max(r['max_us'], float(row['MaxNs']) / 1e3)
    for r in out.values():
        r['avg_us'] = r['total_us'] / max(1, r['calls'])
    return out


def last_json_line(text):
    for line in reversed(text.strip().split('\n')):
        if line.startswith('{'):
            return json.loads(line)
    raise RuntimeError('no JSON line in:\n' + text[-2000:])


def driver(a):
    here = os.path.abspath(__file__)
    runs = {'a': [], 'b': [], 'c': []}
    common = ['--rays', str(a.rays), '--steps', str(a.steps), '--warmup', str(a.warmup)]
    if a.parent_tree:
        runs['parent_a'] = []
    for rep in range(a.repeat):
        for tag in runs:
            if tag == 'parent_a':
                tree = os.path.abspath(a.parent_tree)
                cmd = [sys.executable, os.path.join(tree, 'tools', 'spectrum_broadening_profile.py'), '--turb', '1', '--motion', '0'] + common
                cwd = tree
            else:
                cmd, cwd = [sys.executable, here, '--worker', tag] + common, ROOT
            r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.process_timeout)
            if r.returncode != 0:
                raise SystemExit('spectrum_moments_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            print('rep %d  %-8s %.4f ms per sweep (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_sweep_median'], rec['ms_min'], rec['ms_max']),
                  flush=True)
    result = {'workload': 'radial_d3_turb_fft256 as a PPI: %d rays x %d gates x %d bins, one sub-beam' %
                          (a.rays, runs['a'][0]['n_gates'], runs['a'][0]['n_vbins']),
              'method': 'blocking calls with page-locked outputs, %d steps after %d warm-up calls per process, %d fresh processes per '
                        'call, alternating' % (a.steps, a.warmup, a.repeat),
              'not_measured': 'sub-beam volumes, longer spectra, several lanes in flight, device-resident outputs, a partial field list',
              'calls': {}}
    for tag, recs in runs.items():
        med = [r['ms_per_sweep_median'] for r in recs]
        c = {'ms_per_sweep_median_of_processes': float(np.median(med)), 'ms_per_sweep_medians': med,
             'spread': float((max(med) - min(med)) / np.median(med))}
        for k in ('bytes_handed_over', 'spectrum_checksum', 'width_nanmean', 'kurtosis_nanmedian', 'gates_with_moments'):
            if k in recs[0]:
                c[k] = recs[0][k]
        result['calls'][tag] = c
    ca, cb = result['calls']['a'], result['calls']['b']
    result['b_over_a_ms'] = cb['ms_per_sweep_median_of_processes'] / ca['ms_per_sweep_median_of_processes']
    result['bytes_a_over_b'] = ca['bytes_handed_over'] / cb['bytes_handed_over']
    result['c_over_a_ms'] = result['calls']['c']['ms_per_sweep_median_of_processes'] / ca['ms_per_sweep_median_of_processes']
    if 'parent_a' in result['calls']:
        pa = result['calls']['parent_a']
        lo = min(ca['ms_per_sweep_medians'] + pa['ms_per_sweep_medians'])
        hi = max(ca['ms_per_sweep_medians'] + pa['ms_per_sweep_medians'])
        result['a_over_parent_a_ms'] = ca['ms_per_sweep_median_of_processes'] / pa['ms_per_sweep_median_of_processes']
        # inside the run-to-run spread of the two: the median of each lies inside the range the other's processes span
        result['a_inside_spread_of_parent_a'] = bool(
            min(pa['ms_per_sweep_medians']) <= ca['ms_per_sweep_median_of_processes'] <= max(pa['ms_per_sweep_medians'])
            or min(ca['ms_per_sweep_medians']) <= pa['ms_per_sweep_median_of_processes'] <= max(ca['ms_per_sweep_medians']))
        result['a_and_parent_a_range_ms'] = [lo, hi]
        if 'spectrum_checksum' in pa:
            result['a_checksum_equals_parent'] = bool(pa['spectrum_checksum'] == ca['spectrum_checksum'])
    tables = {}
    for tag, path in (('a', a.kernel_stats_a), ('b', a.kernel_stats_b), ('parent_a', a.kernel_stats_parent)):
        if path:
            tables[tag] = kernel_table(path)
    if tables:
        result['kernels'] = {}
    if 'b' in tables:
        tb = tables['b']
        total = sum(r['total_us'] for r in tb.values())
        per_sweep = {k: r['total_us'] / max(1, tb['k_spec_final']['calls']) for k, r in tb.items()} if 'k_spec_final' in tb else {}
        result['kernels']['b'] = tb
        if 'k_spec_moments' in tb:
            result['kernels']['k_spec_moments_avg_us'] = tb['k_spec_moments']['avg_us']
            result['kernels']['k_spec_moments_share_of_kernel_time'] = tb['k_spec_moments']['total_us'] / total
            result['kernels']['kernel_us_per_sweep_b'] = float(sum(per_sweep.values()))
    if 'a' in tables and 'parent_a' in tables:
        la = {k: r['calls'] for k, r in tables['a'].items()}
        lp = {k: r['calls'] for k, r in tables['parent_a'].items()}
        result['kernels']['a_kernel_calls'] = la
        result['kernels']['parent_a_kernel_calls'] = lp
        result['kernels']['a_same_kernel_list_and_calls_as_parent'] = bool(la == lp)
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', choices=('a', 'b', 'c'), default=None, help='one process of one call: prints one JSON line')
    ap.add_argument('--trace', action='store_true', help='with --worker: the warm-up calls alone, for rocprofv3 --kernel-trace')
    ap.add_argument('--rays', type=int, default=360)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeat', type=int, default=5, help='fresh processes per call')
    ap.add_argument('--process-timeout', type=float, default=240.0)
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--kernel-stats-a', default=None)
    ap.add_argument('--kernel-stats-b', default=None)
    ap.add_argument('--kernel-stats-parent', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a)
    else:
        driver(a)


if __name__ == '__main__':
    main()
