#!/usr/bin/env python
"""tools/network_composite_profile.py -- network composites: the gate plane and the source against the radar plane
and against the per-gate hand-over they replace.  A sibling of tools/composite_profile.py and the same form: seeded inputs from
bench.make_inputs('c2') (360 rays x 500 gates), one lane, wall time per call around BLOCKING calls with page-locked outputs (each
ends in a device synchronise), in fresh processes that alternate:

  radar         simulate_rays_composite on the radar plane (the ZH MAX composite on a 1 km grid of +-150 km): the control (a);
  parent_radar  (--parent-tree DIR: a checkout of the parent commit with its library built) the same call with DIR's package;
  geo           the same sweep on the geographic plane (a 0.0125 x 0.01 degree grid over the network's area): the repeat calls,
                and in 'first_call_ms' the first call of the process, which fetches the geometry by one plain call, makes the
                plane coordinates on the host and uploads them (it also pays the first launches of the process);
  net_dev       get_network_composite: 3 radars x 5 elevations folded into one pass, the map alone;
  net_dev_src   the same with the product 'source';
  net_host      the host alternative: the same fifteen sweeps with every per-gate array delivered, then composite.compose with
                composite.plane_xy on the host;
  bench / parent_bench   (--bench) `python bench.py --gpus 1 --steps 20 --warmup 5` of this tree and of DIR: the control (b).

Kernel times come from a run of its own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/network_composite_profile.py --worker forms
(--worker forms: the per-gate arrays of the bench sweep fed through the test hook to k_comp on the radar plane and on the gate
plane, in both lane forms, and to a three-call SOURCE pass, which adds k_comp_merge); pass the statistics file with
--kernel-stats NAME=FILE to have the figures written into the JSON.

NOT measured: several lanes in flight, device-resident outputs and device-resident plane coordinates, more than one field per
call, networks whose radars do not overlap, the 'model' plane (the same kernel; another host function), ensembles on a plane.

  python tools/network_composite_profile.py --repeat 3 --out profiles/network_composite_profile.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from composite_profile import inside, kernel_table, last_json_line, result_bytes      # noqa: E402

N_RAYS = 360
ELEVATIONS = [1.0, 3.0, 5.0, 8.0, 12.0]
RADARS = [(46.5, 7.5, 1000.0), (46.9, 8.6, 1200.0), (46.0, 6.6, 800.0)]
WORKERS = ('radar', 'geo', 'net_dev', 'net_dev_src', 'net_host', 'forms')


def kernel_name(n):
    """k_comp_<radar|gates>_<combined|per_lane>, k_comp_merge, k_comp_finish, or the bare name of another kernel"""
    m = re.search(r'k_compILb([01])ELb([01])E', n)          # (the mangled name, as the profiler's database keeps it)
    if m:
        return 'k_comp_%s_%s' % ('gates' if m.group(2) == '1' else 'radar', 'combined' if m.group(1) == '1' else 'per_lane')
    n = n.split('(')[0]
    if 'k_comp_finish' in n or 'k_comp_merge' in n:
        return 'k_comp_finish' if 'k_comp_finish' in n else 'k_comp_merge'
    if 'k_comp' in n and '<' in n:
        arg = [x.strip() for x in n.split('<', 1)[1].split('>')[0].split(',')]
        on = lambda x: x in ('true', '1', '(bool)1')       # noqa: E731
        if len(arg) == 2:
            return 'k_comp_%s_%s' % ('gates' if on(arg[1]) else 'radar', 'combined' if on(arg[0]) else 'per_lane')
    return n.split('<')[0].strip().split(' ')[-1]


def worker(a):
    tree = os.path.abspath(a.tree)
    for p in (tree, os.path.join(tree, 'tools')):
        sys.path.insert(0, p)
    import bench
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_amd import composite as CP
    conf, hyds, cube, luts = bench.make_inputs('c2')
    az, el = np.arange(float(N_RAYS)), np.full(N_RAYS, 1.0)
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    e = CP.grid(150e3, 1e3)
    radar_spec = CP.Composite('ZH', e, e)
    first_ms = None
    if a.worker == 'radar':
        run = lambda: op.simulate_rays_composite(az, el, radar_spec)
    else:
        lon, lat = 4.0 + 0.0125 * np.arange(601), 44.5 + 0.01 * np.arange(401)
        geo_spec = CP.Composite('ZH', lon, lat, plane='geographic')
        src_spec = CP.Composite('ZH', lon, lat, products=('max', 'source'), plane='geographic')
    if a.worker == 'forms':
        # k_comp on both planes in both lane forms, and a three-call SOURCE pass, through the test hook on the bench sweep's arrays
        res = op.simulate_rays(az, el)
        zh, xy = {'ZH': np.array(res['ZH'])}, CP.plane_xy('geographic', res['lats'], res['lons'])
        for _ in range(max(1, a.warmup)):
            for form in (1, 2):
                op._ctx.composite_fields(zh, res['dist'], res['heights'], az, radar_spec, lane_form=form)
                op._ctx.composite_fields(zh, None, res['heights'], None, geo_spec, lane_form=form, gate_xy=xy)
            for n, s in enumerate((2, 0, 1)):
                op._ctx.composite_fields(zh, None, res['heights'], None, src_spec, phase=(1 if n == 0 else 0) | (2 if n == 2 else 0),
                                         gate_xy=xy, source=s)
        op.close()
        return
    if a.worker == 'geo':
        run = lambda: op.simulate_rays_composite(az, el, geo_spec)
        t0 = time.perf_counter()
        run()
        first_ms = (time.perf_counter() - t0) * 1e3
    elif a.worker in ('net_dev', 'net_dev_src'):
        spec = src_spec if a.worker == 'net_dev_src' else geo_spec
        run = lambda: op.get_network_composite(RADARS, ELEVATIONS, spec, azimuths=az)
    elif a.worker == 'net_host':
        one = CP.Composite('ZH', [0.0, 1.0], [0.0, 1.0])       # (keep_gates: every per-gate array; its one-cell map is not used)

        def run():
            sweeps = [op.simulate_rays_composite(az, np.full(N_RAYS, e_), one, keep_gates=True, pinned=True, lane=i % op.lanes, radar=r)
                      for i, (r, e_) in enumerate((r, e_) for r in RADARS for e_ in ELEVATIONS)]
            for i in range(op.lanes):
                op.wait(i)
            state = None
            for s in sweeps:
                state = CP.compose(geo_spec, {'ZH': s['ZH']}, None, s['heights'], None, state=state,
                                   gate_xy=CP.plane_xy('geographic', s['lats'], s['lons']))
            return {'sweeps': sweeps, 'host_composite': CP.finish(state)}
    for _ in range(a.warmup):
        res = run()
    t = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        res = run()
        t.append((time.perf_counter() - t0) * 1e3)
    out = {'call': a.worker, 'n_rays': N_RAYS, 'n_gates': len(op.constants.RANGE_RADAR), 'steps': a.steps,
           'ms_per_call_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
           'bytes_handed_over': result_bytes(res)}
    if first_ms is not None:
        out['first_call_ms'] = first_ms
        out['plane_store'] = list(op._ctx.composite_plane())
    if a.worker.startswith('net'):
        out['radars'], out['elevations'] = len(RADARS), ELEVATIONS
    w = res.get('host_composite') or res.get('composite')
    n, m = w['count']['ZH'], w['values']['ZH']['max']
    out.update(counted=int(n.sum()), cells_non_empty=int((n > 0).sum()), cells=int(n.size), max_checksum=float(np.nansum(m, dtype=np.float64)))
    if 'source_of_max' in w['values']['ZH']:
        s = w['values']['ZH']['source_of_max']
        out['cells_per_source'] = [int((s == i).sum()) for i in range(len(RADARS))]
    print(json.dumps(out))
    op.close()


def driver(a):
    here = os.path.abspath(__file__)
    tags = ['radar'] + (['parent_radar'] if a.parent_tree else []) + ['geo', 'net_dev', 'net_dev_src', 'net_host']
    if a.bench:
        tags += ['bench'] + (['parent_bench'] if a.parent_tree else [])
    if a.calls:
        tags = [t for t in a.calls.split(',') if t and t != 'none']
    runs = {t: [] for t in tags}
    for rep in range(a.repeat):
        for tag in tags:
            tree = os.path.abspath(a.parent_tree) if tag.startswith('parent_') else ROOT
            if tag.endswith('bench'):
                cmd = [sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5']
            elif tag == 'parent_radar':         # (the parent has no such tool: its composite_profile's call b is the same call)
                cmd = [sys.executable, os.path.join(tree, 'tools', 'composite_profile.py'), '--worker', 'b', '--tree', tree,
                       '--steps', str(a.steps), '--warmup', str(a.warmup), '--members', '0']
            else:
                cmd = [sys.executable, here, '--worker', tag, '--tree', tree, '--steps', str(a.steps if not tag.startswith('net') else a.net_steps),
                       '--warmup', str(a.warmup if not tag.startswith('net') else a.net_warmup)]
            r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.process_timeout)
            if r.returncode != 0:
                raise SystemExit('network_composite_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            if tag.endswith('bench'):
                print('rep %d  %-12s value %.4e gates/s, %.4f ms per step' % (rep, tag, rec['value'], rec['ms_per_step']), flush=True)
            else:
                print('rep %d  %-12s %.4f ms per call (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_call_median'], rec['ms_min'],
                                                                              rec['ms_max']), flush=True)
    result = {'workload': 'bench.make_inputs(c2): %d rays x 500 gates, one lane; the network: radars %s, elevations %s'
                          % (N_RAYS, RADARS, ELEVATIONS),
              'method': 'blocking calls with page-locked outputs, %d steps after %d warm-up calls per process (network calls: %d after %d), '
                        '%d fresh processes per call, alternating' % (a.steps, a.warmup, a.net_steps, a.net_warmup, a.repeat),
              'not_measured': 'several lanes in flight, device-resident outputs and plane coordinates, more than one field per call, '
                              "networks whose radars do not overlap, the 'model' plane, ensembles on a plane",
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
        if 'first_call_ms' in recs[0]:
            c['first_call_ms'] = [r['first_call_ms'] for r in recs]
        for k in ('bytes_handed_over', 'max_checksum', 'counted', 'cells_non_empty', 'cells', 'radars', 'elevations', 'cells_per_source',
                  'plane_store'):
            if k in recs[0]:
                c[k] = recs[0][k]
        result['calls'][tag] = c
    if a.update and a.out and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        old['calls'].update(result['calls'])
        for k in ('kernels',):
            if k in old:
                result[k] = old[k]
        result['calls'] = old['calls']
    calls = result['calls']
    ms = lambda tag: calls[tag]['ms_per_call_median_of_processes']       # noqa: E731
    if 'parent_radar' in calls and 'radar' in calls:
        result['control_radar_plane'] = {
            'radar_over_parent_ms': ms('radar') / ms('parent_radar'),
            'each_median_inside_the_others_range': inside(calls['radar']['ms_per_call_medians'], calls['parent_radar']['ms_per_call_medians']),
            'maps_equal': bool(calls['radar'].get('max_checksum') == calls['parent_radar'].get('max_checksum')
                               and calls['radar'].get('counted') == calls['parent_radar'].get('counted'))}
    if 'parent_bench' in calls and 'bench' in calls:
        b, pb = calls['bench'], calls['parent_bench']
        result['control_bench'] = {'value_over_parent': b['value_median'] / pb['value_median'],
                                   'each_median_inside_the_others_range': inside(b['values'], pb['values'])}
    if 'geo' in calls and 'radar' in calls:
        result['geo_over_radar_ms'] = ms('geo') / ms('radar')
    if 'net_dev' in calls and 'net_host' in calls:
        result['net_dev_over_net_host_ms'] = ms('net_dev') / ms('net_host')
        result['net_maps_equal'] = bool(calls['net_dev'].get('max_checksum') == calls['net_host'].get('max_checksum')
                                        and calls['net_dev'].get('counted') == calls['net_host'].get('counted'))
    if 'net_dev' in calls and 'net_dev_src' in calls:
        result['net_source_over_net_ms'] = ms('net_dev_src') / ms('net_dev')
    for item in a.kernel_stats or []:
        name, path = item.split('=', 1)
        import composite_profile
        composite_profile.kernel_name = kernel_name            # (this tool's kernel names: the plane form and k_comp_merge)
        tb = kernel_table(path)
        result.setdefault('kernels', {})[name] = {k: v for k, v in tb.items() if k.startswith('k_comp')}
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
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--net-steps', type=int, default=6, help='timed calls of a network worker (fifteen sweeps each)')
    ap.add_argument('--net-warmup', type=int, default=2)
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
