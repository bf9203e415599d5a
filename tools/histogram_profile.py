#!/usr/bin/env python
"""tools/histogram_profile.py -- sweep histograms against the per-gate hand-over they replace.

Seeded inputs from bench.make_inputs('c2'): the 360 x 500 bench sweep, one lane; wall time per sweep around BLOCKING calls with
page-locked outputs (each ends in a device synchronise), in fresh processes that alternate:

  a          simulate_rays: every per-gate array delivered;
  b          simulate_rays_histogram(..., ZH by height, 60 x 40 bins from db_edges): the CFAD alone, no per-gate array;
  c          the same with keep_gates=True: both;
  parent_a   (--parent-tree DIR: a checkout of the parent commit with its library built) call (a) with DIR's package: the control
             for "existing calls did not get slower";
  ens_dev    the --members ensemble (the cube and seeded perturbations, form 'shared'): per-member CFADs from the device;
  ens_host   the same ensemble with every member's per-gate arrays delivered, then histogram.count on the host;
  bench / parent_bench   (--bench) `python bench.py --gpus 1 --steps 20 --warmup 5` of this tree and of DIR: the result line.

The bytes handed over are counted from the arrays of the results (the shared gate coordinates are copied once per table set: not
counted).  Kernel times come from runs of their own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/histogram_profile.py --worker b --trace
(a few untimed calls; --worker degenerate: every counting gate in one cell of a 1-D table, the flush of one cell per workgroup;
--worker full: a 16 384-cell table, 126 x 126 bins); pass the kernel statistics files with --kernel-stats NAME=FILE to have
k_hist's figures written into the JSON.

NOT measured: several lanes in flight, device-resident outputs, more than one field per call, rays_per_block > 0 on the single
sweep, sub-beam volumes, the scans.

  python tools/histogram_profile.py --repeat 3 --out profiles/histogram_profile.json
  python tools/histogram_profile.py --worker b            (one process, one JSON line)
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
GEOM = ('lats', 'lons', 'dist', 'heights')
N_RAYS = 360


def result_bytes(res):
    """bytes of the arrays a call copied to the host"""
    keys = list(res.keys())
    n = 0
    for k in keys:
        if k in GEOM or (k == 'mask' and 'mask_sum8' in keys):
            continue
        if isinstance(res[k], np.ndarray):
            n += res[k].nbytes
    for a in res.get('histogram', {}).get('counts', {}).values():
        n += a.nbytes
    return int(n)


def worker(a):
    tree = os.path.abspath(a.tree)
    for p in (tree, os.path.join(tree, 'tools')):
        sys.path.insert(0, p)
    import bench
    from cosmo_pol_amd import RadarOperator
    from timed_profile import perturbed
    conf, hyds, cube, luts = bench.make_inputs('c2')
    az, el = np.arange(float(N_RAYS)), np.full(N_RAYS, 1.0)
    grid = (cube['zlevels'], cube['proj_info'], cube['resolution'])
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    ens = a.worker in ('ens_dev', 'ens_host')
    if ens:
        op.load_model_ensemble([cube['data']] + [perturbed(cube['data'], 100 + m) for m in range(1, a.members)], *grid)
    else:
        op.load_model_arrays(cube['data'], *grid)
    spec = None
    if a.worker != 'a':
        from cosmo_pol_amd import histogram as HG
        heights = np.linspace(0.0, 12000.0, 41)
        if a.worker == 'degenerate':
            spec = HG.Histogram({'ZH': [0.0, 1e30]})
        elif a.worker == 'full':
            spec = HG.Histogram({'ZH': HG.db_edges(-30, 33, 0.5)}, ordinate='heights', ordinate_edges=np.linspace(0.0, 12000.0, 127))
            assert spec.cells == 16384
        else:
            spec = HG.Histogram({'ZH': HG.db_edges(-10, 50, 1)}, ordinate='heights', ordinate_edges=heights)
    if a.worker == 'a':
        run = lambda: op.simulate_rays(az, el)
    elif a.worker == 'ens_dev':
        run = lambda: op.simulate_rays_ensemble_histogram(az, el, spec)
    elif a.worker == 'ens_host':
        def run():
            res = op.simulate_rays_ensemble(az, el, form='shared')
            res['host_counts'] = HG.count(res, spec, rays_per_block=N_RAYS)
            return res
    else:
        run = lambda: op.simulate_rays_histogram(az, el, spec, keep_gates=a.worker == 'c')
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
    out = {'call': a.worker, 'n_rays': N_RAYS, 'n_gates': len(op.constants.RANGE_RADAR), 'steps': a.steps,
           'ms_per_sweep_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
           'bytes_handed_over': result_bytes(res)}
    if ens:
        out['members'] = a.members
    if 'ZH' in res:
        out['zh_checksum'] = float(np.nansum(res['ZH'], dtype=np.float64))
    counts = res.get('host_counts') or res.get('histogram', {}).get('counts')
    if counts:
        c = counts['ZH']
        out['counted'] = int(c.sum())
        out['cells_non_zero'] = int((c > 0).sum())
        out['cells'] = int(c.size)
    print(json.dumps(out))
    op.close()


def kernel_table_db(path):
    """the same from the database rocprofv3 writes where it writes no CSV (rocpd: one row per dispatch)"""
    import sqlite3
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute('pragma table_info(rocpd_info_kernel_symbol)')]
    name = 'kernel_name' if 'kernel_name' in cols else [c for c in cols if 'name' in c][0]
    out = {}
    for n, t0, t1, grid, wg, lds in db.execute('select s.%s, d.start, d.end, d.grid_size_x, d.workgroup_size_x, d.group_segment_size '
                                               'from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id' % name):
        n = n.split('(')[0]
        n = 'k_hist' if 'k_hist' in n else n.split('<')[0].split(' ')[-1]
        r = out.setdefault(n, {'calls': 0, 'total_us': 0.0, 'min_us': float('inf'), 'max_us': 0.0})
        us = (t1 - t0) / 1e3
        r['calls'] += 1
        r['total_us'] += us
        r['min_us'], r['max_us'] = min(r['min_us'], us), max(r['max_us'], us)
        r['workgroups'], r['lds_bytes'] = grid // max(wg, 1), lds
    for r in out.values():
        r['avg_us'] = r['total_us'] / max(1, r['calls'])
    return out


def kernel_table(path):
    """{kernel: {'calls', 'total_us', 'avg_us', 'min_us', 'max_us'}} from rocprofv3's kernel statistics (names cut at the first
    bracket or parenthesis: template and argument lists away)"""
    if path.endswith('.db'):
        return kernel_table_db(path)
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name', '').split('(')[0].split('<')[0].strip().split(' ')[-1]
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


def inside(x, y):
    """each median inside the other's run-to-run range"""
    return bool(min(y) <= float(np.median(x)) <= max(y) and min(x) <= float(np.median(y)) <= max(x))


def driver(a):
    here = os.path.abspath(__file__)
    tags = ['a', 'b', 'c']
    if a.parent_tree:
        tags.insert(1, 'parent_a')
    if a.members:
        tags += ['ens_dev', 'ens_host']
    if a.bench:
        tags += ['bench'] + (['parent_bench'] if a.parent_tree else [])
    if a.calls:
        tags = [t for t in a.calls.split(',') if t and t != 'none']       # (none: only --kernel-stats, with --update)
    runs = {t: [] for t in tags}
    common = ['--steps', str(a.steps), '--warmup', str(a.warmup), '--members', str(a.members or 0)]
    for rep in range(a.repeat):
        for tag in tags:
            tree = os.path.abspath(a.parent_tree) if tag.startswith('parent_') else ROOT
            if tag.endswith('bench'):
                cmd = [sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5']
            else:
                cmd = [sys.executable, here, '--worker', tag.replace('parent_', ''), '--tree', tree] + common
            r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.process_timeout)
            if r.returncode != 0:
                raise SystemExit('histogram_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            if tag.endswith('bench'):
                print('rep %d  %-12s value %.4e gates/s, %.4f ms per step' % (rep, tag, rec['value'], rec['ms_per_step']), flush=True)
            else:
                print('rep %d  %-12s %.4f ms per sweep (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_sweep_median'], rec['ms_min'],
                                                                               rec['ms_max']), flush=True)
    result = {'workload': 'bench.make_inputs(c2): %d rays x 500 gates, one lane' % N_RAYS,
              'method': 'blocking calls with page-locked outputs, %d steps after %d warm-up calls per process, %d fresh processes per '
                        'call, alternating' % (a.steps, a.warmup, a.repeat),
              'not_measured': 'several lanes in flight, device-resident outputs, more than one field per call, rays_per_block > 0 on '
                              'the single sweep, sub-beam volumes, the scans',
              'calls': {}}
    for tag, recs in runs.items():
        if tag.endswith('bench'):
            v = [r['value'] for r in recs]
            result['calls'][tag] = {'value_median': float(np.median(v)), 'values': v, 'ms_per_step': [r['ms_per_step'] for r in recs],
                                    'spread': float((max(v) - min(v)) / np.median(v))}
            continue
        med = [r['ms_per_sweep_median'] for r in recs]
        c = {'ms_per_sweep_median_of_processes': float(np.median(med)), 'ms_per_sweep_medians': med,
             'spread': float((max(med) - min(med)) / np.median(med))}
        for k in ('bytes_handed_over', 'zh_checksum', 'counted', 'cells_non_zero', 'cells', 'members'):
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
    ca = result['calls'].get('a')
    if ca and 'b' in result['calls'] and 'c' in result['calls']:
        cb, cc = result['calls']['b'], result['calls']['c']
        result['b_over_a_ms'] = cb['ms_per_sweep_median_of_processes'] / ca['ms_per_sweep_median_of_processes']
        result['c_over_a_ms'] = cc['ms_per_sweep_median_of_processes'] / ca['ms_per_sweep_median_of_processes']
        result['bytes_a_over_b'] = ca['bytes_handed_over'] / cb['bytes_handed_over']
    if 'ens_dev' in result['calls'] and 'ens_host' in result['calls']:
        result['ens_dev_over_ens_host_ms'] = (result['calls']['ens_dev']['ms_per_sweep_median_of_processes']
                                              / result['calls']['ens_host']['ms_per_sweep_median_of_processes'])
        result['ens_counts_equal'] = bool(result['calls']['ens_dev'].get('counted') == result['calls']['ens_host'].get('counted'))
    if 'parent_a' in result['calls'] and ca:
        pa = result['calls']['parent_a']
        result['control_sweep'] = {'a_over_parent_a_ms': ca['ms_per_sweep_median_of_processes'] / pa['ms_per_sweep_median_of_processes'],
                                   'each_median_inside_the_others_range': inside(ca['ms_per_sweep_medians'], pa['ms_per_sweep_medians']),
                                   'checksum_equal': bool(pa.get('zh_checksum') == ca.get('zh_checksum'))}
    if 'parent_bench' in result['calls'] and 'bench' in result['calls']:
        b, pb = result['calls']['bench'], result['calls']['parent_bench']
        result['control_bench'] = {'value_over_parent': b['value_median'] / pb['value_median'],
                                   'each_median_inside_the_others_range': inside(b['values'], pb['values'])}
    for item in a.kernel_stats or []:
        name, path = item.split('=', 1)
        tb = kernel_table(path)
        rec = {'k_hist': tb.get('k_hist'), 'kernels': sorted(k for k in tb if k.startswith('k_') or '_k_' in k)}
        if 'k_superob' in tb:
            rec['k_superob'] = tb['k_superob']
        result.setdefault('kernels', {})[name] = rec
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', choices=('a', 'b', 'c', 'degenerate', 'full', 'ens_dev', 'ens_host'), default=None,
                    help='one process of one call: prints one JSON line')
    ap.add_argument('--tree', default=ROOT, help='with --worker: the checkout whose package and bench inputs are used')
    ap.add_argument('--trace', action='store_true', help='with --worker: the warm-up calls alone, for rocprofv3 --kernel-trace')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--members', type=int, default=21, help='members of the ensemble pair (0: no ensemble pair)')
    ap.add_argument('--repeat', type=int, default=3, help='fresh processes per call')
    ap.add_argument('--calls', default=None, help='the calls of this session of the driver, comma-separated (default: all that apply)')
    ap.add_argument('--update', action='store_true', help='join the calls of this session to those --out already holds')
    ap.add_argument('--bench', action='store_true', help="bench.py's result line too (of the parent tree as well)")
    ap.add_argument('--process-timeout', type=float, default=400.0)
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--kernel-stats', action='append', default=None, metavar='NAME=FILE')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a)
    else:
        driver(a)


if __name__ == '__main__':
    main()
