#!/usr/bin/env python
"""tools/composite_profile.py -- gridded composites against the per-gate hand-over they replace.

Seeded inputs from bench.make_inputs('c2'): the 360 x 500 bench sweep, one lane; wall time per call around BLOCKING calls with
page-locked outputs (each ends in a device synchronise), in fresh processes that alternate:

  a          simulate_rays: every per-gate array delivered;
  b          simulate_rays_composite(..., the ZH MAX composite on a 1 km grid of +-150 km): the map alone, no per-gate array;
  c          the same with keep_gates=True: both;
  parent_a   (--parent-tree DIR: a checkout of the parent commit with its library built) call (a) with DIR's package: the control
             for "existing calls did not get slower";
  vol_dev    the 5-elevation volume through get_PPI_composite: one pass, the map alone;
  vol_host   the same five sweeps with every per-gate array delivered (get_PPI's lanes), then composite.compose on the host;
  ens_dev    the --members ensemble (the cube and seeded perturbations, form 'shared'): per-member maps from the device;
  bench / parent_bench   (--bench) `python bench.py --gpus 1 --steps 20 --warmup 5` of this tree and of DIR: the result line.

The bytes handed over are counted from the arrays of the results (the shared gate coordinates are copied once per table set: not
counted).  Kernel times come from runs of their own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/composite_profile.py --worker forms --trace
(--worker forms: the per-gate arrays of the bench sweep fed to k_comp through the test hook in BOTH lane forms -- lanes that
share a cell combined inside the wavefront, and every lane on its own -- for the MAX composite and for every product at once);
pass the kernel statistics files with --kernel-stats NAME=FILE to have k_comp's and k_comp_finish's figures written into the JSON.

NOT measured: several lanes in flight, device-resident outputs, more than one field per call on the single sweep, rays_per_block > 0
on the single sweep, sub-beam volumes, the ensemble's per-gate hand-over.

--layers: height layers and the column.  The 5-elevation volume on the 300 x 300 grid with 20 layers of 500 m,
ZH with composite.vil_table(), written to profiles/composite_layers_profile.json:

  lay_dev    get_PPI_composite with the layered spec: ONE pass gives the 20 CAPPIs and the VIL;
  lay_slabs  what the library offered before for the same result: 20 get_PPI_composite passes, one height_range slab each, then
             composite.column_of on the host over the stacked maps (the slabs' planes are bit for bit the layers': 'stack_equal');
  b / parent_b, bench / parent_bench   the controls: the plain simulate_rays_composite call and bench.py's line, this tree and DIR.

Kernel times of the layered k_comp against the plain one, and of k_comp_column, from
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/composite_profile.py --worker lay_forms --trace
(the five sweeps of the volume fed through the test hook: plain and layered spec, both lane forms).

--sums: the exact sums (the product 'sum').  The ZH composite on the 300 x 300 grid with ('max', 'sum') under
objects.zr_table() -- the mean rain rate per cell -- written to profiles/composite_sums_profile.json:

  sum_dev / b          simulate_rays_composite with ('max', 'sum') against the same call with ('max',): the map alone;
  sum_host             what a user did before: simulate_rays (every per-gate array), then the weight and np.bincount(weights=) on the host;
  sum_vol_dev / vol_dev / sum_vol_host     the same three for the 5-elevation volume (get_PPI_composite; get_PPI's lanes and one bincount);
  sum_ens_dev / ens_dev / sum_ens_host     the same three for the --members ensemble, one map per member;
  b / parent_b, bench / parent_bench       the controls: the plain composite call and bench.py's line, this tree and DIR.

Kernel times of k_comp_sum in both lane forms and of k_comp_sum_finish, beside k_comp's, from
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/composite_profile.py --worker sum_forms --trace
(the bench sweep's arrays through the test hook); the kernel list and launch counts of a call without 'sum' from the same kind of
run of --worker b in this tree and in DIR (--kernel-stats control=FILE, parent_control=FILE: 'control_kernels_equal').

  python tools/composite_profile.py --repeat 3 --out profiles/composite_profile.json
  python tools/composite_profile.py --layers --repeat 3 --parent-tree DIR --bench
  python tools/composite_profile.py --worker b            (one process, one JSON line)
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
ELEVATIONS = [1.0, 3.0, 5.0, 8.0, 12.0]
WORKERS = ('a', 'b', 'c', 'vol_dev', 'vol_host', 'ens_dev', 'forms', 'lay_dev', 'lay_slabs', 'lay_forms',
           'sum_dev', 'sum_host', 'sum_vol_dev', 'sum_vol_host', 'sum_ens_dev', 'sum_ens_host', 'sum_forms')
LAYER_EDGES = [500.0 * j for j in range(21)]          # 20 layers of 500 m


def result_bytes(res):
    """bytes of the arrays a call copied to the host"""
    if isinstance(res, list):
        return sum(result_bytes(r) for r in res)
    keys = list(res.keys())
    n = 0
    for k in keys:
        if k in GEOM or (k == 'mask' and 'mask_sum8' in keys):
            continue
        if isinstance(res[k], np.ndarray):
            n += res[k].nbytes
    w = res.get('composite', {})
    for planes in w.get('values', {}).values():
        n += sum(a.nbytes for a in planes.values())
    n += sum(a.nbytes for a in w.get('count', {}).values())
    for q in ('column', 'column_layers', 'sum', 'sum_skipped'):
        n += sum(a.nbytes for a in w.get(q, {}).values())
    for s in res.get('sweeps', []):
        n += result_bytes(s)
    return int(n)


def worker(a):
    tree = os.path.abspath(a.tree)
    for p in (tree, os.path.join(tree, 'tools')):
        sys.path.insert(0, p)
    import bench
    from cosmo_pol_amd import RadarOperator
    conf, hyds, cube, luts = bench.make_inputs('c2')
    az, el = np.arange(float(N_RAYS)), np.full(N_RAYS, 1.0)
    grid = (cube['zlevels'], cube['proj_info'], cube['resolution'])
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    if a.worker in ('ens_dev', 'sum_ens_dev', 'sum_ens_host'):
        from timed_profile import perturbed
        op.load_model_ensemble([cube['data']] + [perturbed(cube['data'], 100 + m) for m in range(1, a.members)], *grid)
    else:
        op.load_model_arrays(cube['data'], *grid)
    spec = None
    if a.worker != 'a':
        from cosmo_pol_amd import composite as CP
        e = CP.grid(150e3, 1e3)
        spec = CP.Composite('ZH', e, e)
    if a.worker == 'forms':
        # both lane forms of k_comp on the bench sweep's own arrays, through the test hook (the kernels alone are of interest)
        res = op.simulate_rays(az, el)
        every = CP.Composite('ZH', e, e, products=('max', 'lowest', 'echo_top'), thresholds=CP.from_db([18.0, 35.0]))
        for _ in range(max(1, a.warmup)):
            for form in (1, 2):
                for s in (spec, every):
                    op._ctx.composite_fields({'ZH': np.array(res['ZH'])}, res['dist'], res['heights'], az, s, lane_form=form)
        op.close()
        return
    if a.worker.startswith('sum_'):
        from cosmo_pol_amd import objects as OB
        zr = OB.zr_table()
        summed = CP.Composite('ZH', e, e, products=('max', 'sum'), weight={'ZH': zr})
        rs, rc = CP.ray_tables(az)

        def host_sums(zh, dist):
            """the mean rain rate per cell on the host: the weight of every gate, the cell of every gate, np.bincount(weights=)"""
            d = np.asarray(dist, dtype=np.float64)
            ix = np.searchsorted(e, d * rs[:, None], side='right') - 1
            iy = np.searchsorted(e, d * rc[:, None], side='right') - 1
            cells = (len(e) - 1) ** 2
            cell = iy * (len(e) - 1) + ix
            out = []
            for m in np.asarray(zh).reshape(-1, *d.shape):
                w = OB.weight_of(m, zr)
                ok = np.isfinite(w) & (d == d) & (ix >= 0) & (ix < len(e) - 1) & (iy >= 0) & (iy < len(e) - 1)
                out.append((np.bincount(cell[ok], weights=w[ok].astype(np.float64), minlength=cells), np.bincount(cell[ok], minlength=cells)))
            return out
    if a.worker == 'sum_forms':
        # both lane forms of k_comp_sum (and of k_comp) on the bench sweep's own arrays, through the test hook
        res = op.simulate_rays(az, el)
        for _ in range(max(1, a.warmup)):
            for form in (1, 2):
                op._ctx.composite_fields({'ZH': np.array(res['ZH'])}, res['dist'], res['heights'], az, summed, lane_form=form)
        op.close()
        return
    if a.worker.startswith('lay_'):
        layered = CP.Composite('ZH', e, e, products=('max', 'column'), z_edges=LAYER_EDGES, column={'ZH': CP.vil_table()})
    if a.worker == 'lay_forms':
        # the volume's five sweeps through the test hook: the plain MAX composite and the layered one, both lane forms
        sweeps = [op.simulate_rays(az, np.full(N_RAYS, e_)) for e_ in ELEVATIONS]
        for _ in range(max(1, a.warmup)):
            for form in (1, 2):
                for s in (spec, layered):
                    for i, r in enumerate(sweeps):
                        op._ctx.composite_fields({'ZH': np.array(r['ZH'])}, r['dist'], r['heights'], az, s, lane_form=form,
                                                 phase=(1 if i == 0 else 0) | (2 if i == len(sweeps) - 1 else 0))
        op.close()
        return
    if a.worker == 'lay_dev':
        run = lambda: op.get_PPI_composite(ELEVATIONS, layered, azimuths=az)
    elif a.worker == 'lay_slabs':
        slabs = [CP.Composite('ZH', e, e, height_range=(LAYER_EDGES[l], LAYER_EDGES[l + 1])) for l in range(len(LAYER_EDGES) - 1)]

        def run():
            maps = [op.get_PPI_composite(ELEVATIONS, s, azimuths=az)['composite'] for s in slabs]
            stack = np.stack([m['values']['ZH']['max'] for m in maps], axis=1)
            col, lay = CP.column_of(layered, stack)
            return {'composite': {'values': {'ZH': {'max': stack, 'height_of_max': np.stack([m['values']['ZH']['height_of_max'] for m in maps], axis=1)}},
                                  'count': {'ZH': np.stack([m['count']['ZH'] for m in maps], axis=1)}, 'column': {'ZH': col},
                                  'column_layers': {'ZH': lay}}}
    elif a.worker == 'sum_dev':
        run = lambda: op.simulate_rays_composite(az, el, summed)
    elif a.worker == 'sum_vol_dev':
        run = lambda: op.get_PPI_composite(ELEVATIONS, summed, azimuths=az)
    elif a.worker == 'sum_ens_dev':
        run = lambda: op.simulate_rays_ensemble_composite(az, el, summed)
    elif a.worker == 'sum_host':
        def run():
            res = op.simulate_rays(az, el)
            res['host_sums'] = host_sums(res['ZH'], res['dist'])
            return res
    elif a.worker == 'sum_ens_host':
        def run():
            res = op.simulate_rays_ensemble(az, el)
            res['host_sums'] = host_sums(res['ZH'], res['dist'])
            return res
    elif a.worker == 'sum_vol_host':
        def run():
            sweeps = [op.simulate_rays(az, np.full(N_RAYS, e_), pinned=True, lane=i % op.lanes) for i, e_ in enumerate(ELEVATIONS)]
            for i in range(op.lanes):
                op.wait(i)
            parts = [host_sums(s['ZH'], s['dist'])[0] for s in sweeps]
            return {'sweeps': sweeps, 'host_sums': [(sum(p[0] for p in parts), sum(p[1] for p in parts))]}
    elif a.worker == 'a':
        run = lambda: op.simulate_rays(az, el)
    elif a.worker == 'ens_dev':
        run = lambda: op.simulate_rays_ensemble_composite(az, el, spec)
    elif a.worker == 'vol_dev':
        run = lambda: op.get_PPI_composite(ELEVATIONS, spec, azimuths=az)
    elif a.worker == 'vol_host':
        def run():
            sweeps = [op.simulate_rays(az, np.full(N_RAYS, e_), pinned=True, lane=i % op.lanes) for i, e_ in enumerate(ELEVATIONS)]
            for i in range(op.lanes):
                op.wait(i)
            state = None
            for s in sweeps:
                state = CP.compose(spec, {'ZH': s['ZH']}, s['dist'], s['heights'], az, state=state)
            return {'sweeps': sweeps, 'host_composite': CP.finish(state)}
    else:
        run = lambda: op.simulate_rays_composite(az, el, spec, keep_gates=a.worker == 'c')
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
           'ms_per_call_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
           'bytes_handed_over': result_bytes(res)}
    if 'ens' in a.worker:
        out['members'] = a.members
    if 'host_sums' in res:
        out['host_sum_total'] = float(sum(t.sum() for t, _ in res['host_sums']))
        out['summed'] = int(sum(n.sum() for _, n in res['host_sums']))
    if 'vol' in a.worker:
        out['elevations'] = ELEVATIONS
    if 'ZH' in res:
        out['zh_checksum'] = float(np.nansum(res['ZH'], dtype=np.float64))
    w = res.get('host_composite') or res.get('composite')
    if w:
        n, m = w['count']['ZH'], w['values']['ZH']['max']
        out['counted'] = int(n.sum())
        out['cells_non_empty'] = int((n > 0).sum())
        out['cells'] = int(n.size)
        out['max_checksum'] = float(np.nansum(m, dtype=np.float64))
        if 'sum' in w:
            out['sum_total'] = float(np.nansum(w['sum']['ZH']))
            out['summed'] = int(n.sum()) - int(np.asarray(w['sum_skipped']['ZH'], dtype=np.int64).sum())
            mean = CP.mean_of(w, 'ZH')
            out['mean_rain_rate_max_mm_h'] = float(np.nanmax(mean))
            out['sum_bits_xor'] = int(np.bitwise_xor.reduce(np.ascontiguousarray(w['sum']['ZH']).view(np.uint64).ravel()))
        if 'column' in w:
            col = np.ascontiguousarray(w['column']['ZH'])
            out['column_cells'] = int(np.isfinite(col).sum())
            out['column_max_kg_m2'] = float(np.nanmax(col))
            out['column_bits_xor'] = int(np.bitwise_xor.reduce(col.view(np.uint64).ravel()))       # (equal bits give equal words)
            out['column_layers_sum'] = int(np.asarray(w['column_layers']['ZH'], dtype=np.int64).sum())
            out['stack_bits_xor'] = int(np.bitwise_xor.reduce(np.ascontiguousarray(m).view(np.uint32).ravel()))
    print(json.dumps(out))
    op.close()


def kernel_name(n):
    """k_comp_finish, k_comp_combined (the wavefront combine), k_comp_per_lane, or the bare name of another kernel"""
    n = n.split('(')[0]
    for plain in ('k_comp_sum_finish', 'k_comp_finish', 'k_comp_column', 'k_comp_merge'):
        if plain in n:
            return plain
    if 'k_comp_sum' in n:
        # k_comp_sum<COMBINE, GATES, LAYERS>
        args = [x.strip() for x in (n.split('<', 1)[1].split('>')[0] if '<' in n else '').split(',')]
        on = lambda i: len(args) > i and args[i] in ('true', '1')       # noqa: E731
        return ('k_comp_sum_combined' if on(0) else 'k_comp_sum_per_lane') + ('_layers' if on(2) else '')
    if 'k_comp' in n:
        # k_comp<COMBINE, GATES, LAYERS>: the first argument names the lane form, the third the layered instantiation
        args = [x.strip() for x in (n.split('<', 1)[1].split('>')[0] if '<' in n else '').split(',')]
        on = lambda i: len(args) > i and args[i] in ('true', '1')       # noqa: E731
        return ('k_comp_combined' if on(0) else 'k_comp_per_lane') + ('_layers' if on(2) else '')
    return n.split('<')[0].strip().split(' ')[-1]


def kernel_table_db(path):
    """the same from the database rocprofv3 writes where it writes no CSV (rocpd: one row per dispatch)"""
    import sqlite3
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute('pragma table_info(rocpd_info_kernel_symbol)')]
    name = 'kernel_name' if 'kernel_name' in cols else [c for c in cols if 'name' in c][0]
    out = {}
    for n, t0, t1, grid, wg, lds in db.execute('select s.%s, d.start, d.end, d.grid_size_x, d.workgroup_size_x, d.group_segment_size '
                                               'from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id' % name):
        r = out.setdefault(kernel_name(n), {'calls': 0, 'total_us': 0.0, 'min_us': float('inf'), 'max_us': 0.0})
        us = (t1 - t0) / 1e3
        r['calls'] += 1
        r['total_us'] += us
        r['min_us'], r['max_us'] = min(r['min_us'], us), max(r['max_us'], us)
        r['workgroups'], r['lds_bytes'] = grid // max(wg, 1), lds
    for r in out.values():
        r['avg_us'] = r['total_us'] / max(1, r['calls'])
    return out


def kernel_table(path):
    """{kernel: {'calls', 'total_us', 'avg_us', 'min_us', 'max_us'}} from rocprofv3's kernel statistics"""
    if path.endswith('.db'):
        return kernel_table_db(path)
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = kernel_name(row.get('Name', ''))
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
    tags = ['a', 'b', 'c', 'vol_dev', 'vol_host']
    if a.parent_tree:
        tags.insert(1, 'parent_a')
    if a.members:
        tags += ['ens_dev']
    if a.layers:
        tags = ['lay_dev', 'lay_slabs', 'b'] + (['parent_b'] if a.parent_tree else [])
        a.out = a.out or os.path.join(ROOT, 'profiles', 'composite_layers_profile.json')
    if a.sums:
        tags = ['sum_dev', 'b', 'sum_host', 'sum_vol_dev', 'vol_dev', 'sum_vol_host'] + (['sum_ens_dev', 'ens_dev', 'sum_ens_host'] if a.members else []) \
            + (['parent_b'] if a.parent_tree else [])
        a.out = a.out or os.path.join(ROOT, 'profiles', 'composite_sums_profile.json')
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
                raise SystemExit('composite_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            if tag.endswith('bench'):
                print('rep %d  %-12s value %.4e gates/s, %.4f ms per step' % (rep, tag, rec['value'], rec['ms_per_step']), flush=True)
            else:
                print('rep %d  %-12s %.4f ms per call (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_call_median'], rec['ms_min'],
                                                                              rec['ms_max']), flush=True)
    result = {'workload': 'bench.make_inputs(c2): %d rays x 500 gates, one lane; the volume: elevations %s' % (N_RAYS, ELEVATIONS),
              'method': 'blocking calls with page-locked outputs, %d steps after %d warm-up calls per process, %d fresh processes per '
                        'call, alternating' % (a.steps, a.warmup, a.repeat),
              'not_measured': 'several lanes in flight, device-resident outputs, more than one field per call on the single sweep, '
                              "rays_per_block > 0 on the single sweep, sub-beam volumes, the ensemble's per-gate hand-over",
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
        for k in ('bytes_handed_over', 'zh_checksum', 'max_checksum', 'counted', 'cells_non_empty', 'cells', 'members', 'elevations',
                  'column_cells', 'column_max_kg_m2', 'column_bits_xor', 'column_layers_sum', 'stack_bits_xor',
                  'sum_total', 'host_sum_total', 'summed', 'mean_rain_rate_max_mm_h', 'sum_bits_xor'):
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
    if all(t in calls for t in ('a', 'b', 'c')):
        result['b_over_a_ms'] = ms('b') / ms('a')
        result['c_over_a_ms'] = ms('c') / ms('a')
        result['bytes_a_over_b'] = calls['a']['bytes_handed_over'] / calls['b']['bytes_handed_over']
    if 'vol_dev' in calls and 'vol_host' in calls:
        result['vol_dev_over_vol_host_ms'] = ms('vol_dev') / ms('vol_host')
        result['vol_maps_equal'] = bool(calls['vol_dev'].get('max_checksum') == calls['vol_host'].get('max_checksum')
                                        and calls['vol_dev'].get('counted') == calls['vol_host'].get('counted'))
    if 'lay_dev' in calls and 'lay_slabs' in calls:
        result['workload'] += '; --layers: the volume on the 300 x 300 grid, %d layers of 500 m, ZH with vil_table()' % (len(LAYER_EDGES) - 1)
        result['lay_dev_over_lay_slabs_ms'] = ms('lay_dev') / ms('lay_slabs')
        result['column_equal'] = bool(all(calls['lay_dev'].get(k) == calls['lay_slabs'].get(k) is not None
                                          for k in ('column_bits_xor', 'column_layers_sum', 'column_cells')))
        result['stack_equal'] = bool(all(calls['lay_dev'].get(k) == calls['lay_slabs'].get(k) is not None
                                         for k in ('stack_bits_xor', 'counted', 'max_checksum')))
    for dev, plain, host, name in (('sum_dev', 'b', 'sum_host', 'sweep'), ('sum_vol_dev', 'vol_dev', 'sum_vol_host', 'volume'),
                                   ('sum_ens_dev', 'ens_dev', 'sum_ens_host', 'ensemble')):
        if all(t in calls for t in (dev, plain, host)):
            if 'workload' in result and '--sums' not in result['workload']:
                result['workload'] += "; --sums: ZH on the 300 x 300 grid, ('max', 'sum') under objects.zr_table()"
            result['sums_' + name] = {'with_sum_over_max_alone_ms': ms(dev) / ms(plain), 'with_sum_minus_max_alone_ms': ms(dev) - ms(plain),
                                      'device_over_host_ms': ms(dev) / ms(host), 'summed_gates_equal': bool(calls[dev].get('summed') == calls[host].get('summed')),
                                      'host_total_minus_exact_total': calls[host].get('host_sum_total', 0.0) - calls[dev].get('sum_total', 0.0)}
    if 'parent_b' in calls and 'b' in calls:
        cb, pb = calls['b'], calls['parent_b']
        result['control_composite'] = {'b_over_parent_b_ms': ms('b') / ms('parent_b'),
                                       'each_median_inside_the_others_range': inside(cb['ms_per_call_medians'], pb['ms_per_call_medians']),
                                       'maps_equal': bool(pb.get('max_checksum') == cb.get('max_checksum') and pb.get('counted') == cb.get('counted'))}
    if 'parent_a' in calls and 'a' in calls:
        ca, pa = calls['a'], calls['parent_a']
        result['control_sweep'] = {'a_over_parent_a_ms': ms('a') / ms('parent_a'),
                                   'each_median_inside_the_others_range': inside(ca['ms_per_call_medians'], pa['ms_per_call_medians']),
                                   'checksum_equal': bool(pa.get('zh_checksum') == ca.get('zh_checksum'))}
    if 'parent_bench' in calls and 'bench' in calls:
        b, pb = calls['bench'], calls['parent_bench']
        result['control_bench'] = {'value_over_parent': b['value_median'] / pb['value_median'],
                                   'each_median_inside_the_others_range': inside(b['values'], pb['values'])}
    for item in a.kernel_stats or []:
        name, path = item.split('=', 1)
        tb = kernel_table(path)
        result.setdefault('kernels', {})[name] = {k: tb.get(k) for k in ('k_comp_combined', 'k_comp_per_lane', 'k_comp_finish')}
        for k in ('k_comp_combined_layers', 'k_comp_per_lane_layers', 'k_comp_column',            # (a run with height layers)
                  'k_comp_sum_combined', 'k_comp_sum_per_lane', 'k_comp_sum_finish'):               # (a run with the exact sums)
            if k in tb:
                result['kernels'][name][k] = tb[k]
        if name in ('control', 'parent_control'):
            # the whole kernel list of a call without 'sum': names and launch counts
            result.setdefault('kernel_lists', {})[name] = {k: v['calls'] for k, v in sorted(tb.items())}
    lists = result.get('kernel_lists', {})
    if 'control' in lists and 'parent_control' in lists:
        result['control_kernels_equal'] = bool(lists['control'] == lists['parent_control'])
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
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--members', type=int, default=21, help='members of the ensemble call (0: none)')
    ap.add_argument('--repeat', type=int, default=3, help='fresh processes per call')
    ap.add_argument('--calls', default=None, help='the calls of this session of the driver, comma-separated (default: all that apply)')
    ap.add_argument('--update', action='store_true', help='join the calls of this session to those --out already holds')
    ap.add_argument('--layers', action='store_true', help='height layers and the column: lay_dev against lay_slabs, the controls b / parent_b; '
                    'writes profiles/composite_layers_profile.json unless --out names another file')
    ap.add_argument('--sums', action='store_true', help="the exact sums: ('max', 'sum') under zr_table against ('max',) and against the host, "
                    'sweep, volume and ensemble; writes profiles/composite_sums_profile.json unless --out names another file')
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
