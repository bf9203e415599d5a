#!/usr/bin/env python
"""tools/object_match_profile.py -- the match of the object cells on the device against intersecting label maps on the host
("match").

The conditions and the protocol of tools/objects_profile.py: seeded inputs from bench.make_inputs('c2'), the 360 x 500 bench sweep,
one lane, an ensemble of --members states; per-member ZH 'max' maps on the 300 x 300 grid of 1 km cells at three thresholds (18,
30, 40 dBZ), scored at radius 0 against the map of member 1; cells under 8-connectivity, min_area 4, 1024 table rows, 4096 piece
rows.  Wall time per call around BLOCKING calls with page-locked outputs, in fresh processes that alternate; the medians of the
processes' medians with their spread:

  ens_cells         (a) simulate_rays_ensemble_composite_fss with an objects.Objects: maps, scores, cells and label maps;
  ens_cells_bare    (a) without the label maps;
  ens_match         (b) ens_cells_bare with match=True: the pieces and `covered` from the device, no label map handed over;
  ens_match_labels  (b) with the label maps too;
  ens_host_match    (c) what a user did before: ens_cells (the label maps copied to the host), then objects.pieces_of_map and
                    objects.pairs in NumPy for every member and threshold;
  parent_ens_cells  ens_cells of --parent-tree DIR (a checkout of the parent commit with its library built): the control for "the
                    call without the match did not get slower"; the margin is the spread of the processes this run reports.

Kernel times come from a run of its own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/object_match_profile.py --worker ens_match --trace
pass the kernel statistics file with --kernel-stats NAME=FILE.

NOT measured: several lanes in flight, device-resident outputs, a domain mask, other grids, connectivities, thresholds and member
counts, the single sweep, a volume, the largest grid, piece tables that overflow.

  python tools/object_match_profile.py --repeat 3 --parent-tree DIR
  python tools/object_match_profile.py --worker ens_match            (one process, one JSON line)

With --track the TRACK of the object cells instead, into profiles/object_track_profile.json: a series of --times
scan times of the same sweep (the model's hydrometeors carried along by one cell north and two cells east per time) through ONE
simulate_rays_at_composite_fss, rays_per_block = 360: one ZH 'max' plane per scan time on the same grid at the same thresholds,
scored at radius 0 against the plane of time 1; cells as above, max_shift 8, 1024 piece rows per pair and threshold:

  series_cells         the call with the label maps, track off;
  series_cells_bare    without the label maps, track off;
  series_track         series_cells_bare with track=True, max_shift=8: correlation, shift, pieces and `covered` from the device;
  series_host_track    what a user did before: series_cells (the label maps copied to the host), then objects.track_of_labels in NumPy;
  parent_series_cells  series_cells of --parent-tree DIR: the control for "the call without the track did not get slower".

  python tools/object_match_profile.py --track --repeat 3 --parent-tree DIR
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from composite_profile import inside, kernel_table, last_json_line  # noqa: E402
from objects_profile import CONNECTIVITY, MAX_OBJECTS, MIN_AREA, N_RAYS, THRESHOLDS_DBZ, handed_bytes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_PIECES = 4096
WORKERS = ('ens_cells', 'ens_cells_bare', 'ens_match', 'ens_match_labels', 'ens_host_match')
TRACK_WORKERS = ('series_cells', 'series_cells_bare', 'series_track', 'series_host_track')
TRACK_KERNELS = ('k_track_bits', 'k_track_corr', 'k_track_shift', 'k_track_runs', 'k_track_attr', 'k_match_decode', 'k_obj_merge', 'k_obj_flatten',
                 'k_obj_area', 'k_obj_count', 'k_obj_number', 'k_obj_runs', 'k_obj_attr', 'k_obj_decode', 'k_frac_rows', 'k_frac_cols', 'k_frac_score',
                 'k_comp_finish')
MAX_SHIFT, MAX_TRACK_PIECES = 8, 1024
KERNELS = ('k_match_runs', 'k_match_attr', 'k_match_decode', 'k_obj_runs', 'k_obj_merge', 'k_obj_flatten', 'k_obj_area', 'k_obj_count',
           'k_obj_number', 'k_obj_attr', 'k_obj_decode', 'k_frac_rows', 'k_frac_cols', 'k_frac_score', 'k_comp_finish')


def host_match(OB, ob, connectivity):
    """The match on the host from the label maps of a result: pieces_of_map and the fold of `pairs` per member and threshold."""
    labels, observed = np.array(ob['labels']), np.array(ob['observed']['labels'])
    n_blocks, n_thr = labels.shape[:2]
    match = (np.zeros((n_blocks, n_thr), np.uint32), np.zeros((n_blocks, n_thr, MAX_PIECES, OB.WORDS), np.uint32),
             np.zeros((n_blocks, n_thr, 2, MAX_OBJECTS), np.uint32))
    for b in range(n_blocks):
        for t in range(n_thr):
            match[0][b, t], match[1][b, t], match[2][b, t] = OB.pieces_of_map(labels[b, t], observed[t], connectivity, MAX_PIECES, MAX_OBJECTS)
    named = dict(ob, pieces={'n_pieces': match[0], 'first': match[1][..., OB.FIRST], 'area': match[1][..., OB.AREA],
                             'sum_x': match[1][..., OB.SUM_X], 'sum_y': match[1][..., OB.SUM_Y], 'bbox': match[1][..., OB.X0:OB.Y1 + 1],
                             'forecast': match[1][..., OB.FORECAST], 'observed': match[1][..., OB.OBSERVED]},
                 covered=match[2][:, :, 0], covered_observed=match[2][:, :, 1])
    n_pairs = sum(OB.pairs(named, b, t)['area'].size for b in range(n_blocks) for t in range(n_thr))
    return named, n_pairs


def carried(data, k):
    """The state `data` with its hydrometeor masses carried along by k cells north and 2 k cells east."""
    return {name: (np.roll(v, (k, 2 * k), axis=(-2, -1)) if name.startswith('Q') else v) for name, v in data.items()}


def track_worker(a):
    tree = os.path.abspath(a.tree)
    for p in (tree, os.path.join(tree, 'tools')):
        sys.path.insert(0, p)
    import bench
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_amd import composite as CP
    from cosmo_pol_amd import neighbourhood as NB
    from cosmo_pol_amd import objects as OB
    conf, hyds, cube, luts = bench.make_inputs('c2')
    n_t = a.times
    az, el = np.tile(np.arange(float(N_RAYS)), n_t), np.full(N_RAYS * n_t, 1.0)
    series = [300.0 * k for k in range(n_t)]
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    op.load_model_series([carried(cube['data'], k) for k in range(n_t)], series, cube['zlevels'], cube['proj_info'], cube['resolution'])
    e = CP.grid(150e3, 1e3)
    cspec = CP.Composite('ZH', e, e)
    spec = NB.Fractions(cspec, 'ZH', CP.from_db(THRESHOLDS_DBZ), [0])
    tt = np.repeat(series, N_RAYS)
    observed = np.array(op.simulate_rays_at_composite(az[:N_RAYS], el[:N_RAYS], series[1], cspec)['composite']['values']['ZH']['max'][0])
    kw = dict(connectivity=CONNECTIVITY, min_area=MIN_AREA, max_objects=MAX_OBJECTS)
    if a.worker == 'series_track':
        kw.update(track=True, max_shift=MAX_SHIFT, max_track_pieces=MAX_TRACK_PIECES)
    ospec = OB.Objects(spec, labels=a.worker in ('series_cells', 'series_host_track'), **kw)
    call = lambda: op.simulate_rays_at_composite_fss(az, el, tt, ospec, observed, rays_per_block=N_RAYS)      # noqa: E731
    if a.worker == 'series_host_track':
        host_spec = OB.Objects(spec, track=True, max_shift=MAX_SHIFT, max_track_pieces=MAX_TRACK_PIECES, **kw)

        def run():
            res = call()
            res['composite']['objects']['track'] = OB.track_result(OB.track_of_labels(host_spec, np.array(res['composite']['objects']['labels'])))
            return res
    else:
        run = call
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
    ob = w['objects']
    out = {'call': a.worker, 'n_rays': N_RAYS, 'n_gates': len(op.constants.RANGE_RADAR), 'steps': a.steps, 'times': n_t,
           'ms_per_call_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
           'max_checksum': float(np.nansum(w['values']['ZH']['max'], dtype=np.float64)),
           'sums_checksum': [int(np.array(w['fractions'][k]).sum(dtype=np.uint64)) for k in ('diff2', 'forecast2', 'observed2')],
           'cells_checksum': [int(np.array(ob[k]).sum(dtype=np.uint64)) for k in ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')],
           'n_objects_per_time': [[int(x) for x in row] for row in np.array(ob['n_objects'])],
           'thresholds_dbz': THRESHOLDS_DBZ, 'terms': [CONNECTIVITY, MIN_AREA, MAX_OBJECTS, MAX_SHIFT, MAX_TRACK_PIECES]}
    if 'track' in ob:
        tr = {k: np.array(v) for k, v in ob['track'].items()}
        out['track_checksum'] = [int(tr[k].astype(np.int64).sum()) for k in ('correlation', 'shift', 'n_pieces', 'pieces', 'covered')]
        out['shift_first_pair'] = [[int(x) for x in row] for row in tr['shift'][0]]
        out['n_pieces_max'] = int(tr['n_pieces'].max())
        out['n_tracks'] = [int(OB.tracks(ob, t)['birth'].size) for t in range(len(THRESHOLDS_DBZ))]
        out['track_bytes'] = int(sum(v.nbytes for v in tr.values()))
    if a.worker != 'series_host_track':
        out['bytes'] = handed_bytes({k: (v if k != 'objects' else {q: r for q, r in v.items() if q != 'track'}) for k, v in w.items()})
    else:
        out['labels_bytes'] = int(np.array(ob['labels']).nbytes + np.array(ob['observed']['labels']).nbytes)
    print(json.dumps(out))
    op.close()


def track_driver(a):
    here = os.path.abspath(__file__)
    tags = list(TRACK_WORKERS) + (['parent_series_cells'] if a.parent_tree else [])
    if a.calls:
        tags = [t for t in a.calls.split(',') if t and t != 'none']
    runs = {t: [] for t in tags}
    common = ['--track', '--steps', str(a.steps), '--warmup', str(a.warmup), '--times', str(a.times)]
    for rep in range(a.repeat):
        for tag in tags:
            tree = os.path.abspath(a.parent_tree) if tag.startswith('parent_') else ROOT
            cmd = [sys.executable, here, '--worker', tag.replace('parent_', ''), '--tree', tree] + common
            r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.process_timeout)
            if r.returncode != 0:
                raise SystemExit('object_match_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            print('rep %d  %-19s %.4f ms per call (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_call_median'], rec['ms_min'], rec['ms_max']), flush=True)
    result = {'workload': 'bench.make_inputs(c2): a series of %d scan times of %d rays x 500 gates in ONE simulate_rays_at_composite_fss, '
                          'rays_per_block %d, one lane; the hydrometeors carried along by (1, 2) cells per time; ZH max planes on 300 x 300 '
                          'cells of 1 km, thresholds %s dBZ, radius 0, observed = the plane of time 1; cells: connectivity %d, min_area %d, %d '
                          'table rows; track: max_shift %d, %d piece rows' % (a.times, N_RAYS, N_RAYS, THRESHOLDS_DBZ, CONNECTIVITY, MIN_AREA,
                                                                             MAX_OBJECTS, MAX_SHIFT, MAX_TRACK_PIECES),
              'method': 'blocking calls with page-locked outputs, %d steps after %d warm-up calls per process, %d fresh processes per '
                        'call, alternating' % (a.steps, a.warmup, a.repeat),
              'not_measured': 'several lanes in flight, device-resident outputs, given shifts, a domain mask, other grids, reaches, '
                              'connectivities, thresholds and series lengths, the largest grid, piece tables that overflow',
              'calls': {}}
    for tag, recs in runs.items():
        med = [r['ms_per_call_median'] for r in recs]
        c = {'ms_per_call_median_of_processes': float(np.median(med)), 'ms_per_call_medians': med,
             'range_ms': [min(med), max(med)], 'spread': float((max(med) - min(med)) / np.median(med))}
        for k in ('max_checksum', 'times', 'sums_checksum', 'n_objects_per_time', 'cells_checksum', 'thresholds_dbz', 'terms', 'bytes',
                  'track_checksum', 'shift_first_pair', 'n_pieces_max', 'n_tracks', 'track_bytes', 'labels_bytes'):
            if k in recs[0]:
                c[k] = recs[0][k]
        result['calls'][tag] = c
    if a.update and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        old['calls'].update(result['calls'])
        for k in ('kernels', 'kernel_lists', 'method', 'workload'):          # (a session that only joins kernel statistics keeps them)
            if k in old and (k in ('kernels', 'kernel_lists') or not runs):
                result[k] = old[k]
        result['calls'] = old['calls']
    calls = result['calls']
    ms = lambda tag: calls[tag]['ms_per_call_median_of_processes']       # noqa: E731
    if 'series_track' in calls and 'series_cells_bare' in calls:
        result['track_cost_ms'] = ms('series_track') - ms('series_cells_bare')
    if 'series_track' in calls and 'series_host_track' in calls:
        result['track_on_device_over_labels_and_host_track_ms'] = [ms('series_track'), ms('series_host_track')]
        result['track_equal'] = bool(calls['series_track'].get('track_checksum') == calls['series_host_track'].get('track_checksum')
                                     and calls['series_track'].get('n_tracks') == calls['series_host_track'].get('n_tracks'))
        result['bytes_handed_over'] = {'device': calls['series_track'].get('track_bytes'), 'host_path_labels': calls['series_host_track'].get('labels_bytes')}
    if 'parent_series_cells' in calls and 'series_cells' in calls:
        cc, pc = calls['series_cells'], calls['parent_series_cells']
        result['control_call_without_track'] = {'series_cells_over_parent_ms': ms('series_cells') / ms('parent_series_cells'),
                                                'range_ms': cc['range_ms'], 'parent_range_ms': pc['range_ms'],
                                                'each_median_inside_the_others_range': inside(cc['ms_per_call_medians'], pc['ms_per_call_medians']),
                                                'checksums_equal': bool(pc.get('max_checksum') == cc.get('max_checksum')
                                                                        and pc.get('sums_checksum') == cc.get('sums_checksum')
                                                                        and pc.get('cells_checksum') == cc.get('cells_checksum'))}
    for item in a.kernel_stats or []:
        name, path = item.split('=', 1)
        tb = kernel_table(path)
        result.setdefault('kernels', {})[name] = {k: tb.get(k) or next((v for n, v in tb.items() if '_Z%d%s' % (len(k), k) in n
                                                                        or re.search(k + r'(?![A-Za-z0-9_])', n)), None) for k in TRACK_KERNELS}
        result.setdefault('kernel_lists', {})[name] = {n: v['calls'] for n, v in sorted(tb.items())}
    lists = result.get('kernel_lists', {})
    if 'series_cells' in lists and 'parent_series_cells' in lists:
        result['control_kernel_list_equals_parent'] = lists['series_cells'] == lists['parent_series_cells']
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


def worker(a):
    tree = os.path.abspath(a.tree)
    for p in (tree, os.path.join(tree, 'tools')):
        sys.path.insert(0, p)
    import bench
    from timed_profile import perturbed
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_amd import composite as CP
    from cosmo_pol_amd import neighbourhood as NB
    from cosmo_pol_amd import objects as OB
    conf, hyds, cube, luts = bench.make_inputs('c2')
    az, el = np.arange(float(N_RAYS)), np.full(N_RAYS, 1.0)
    grid = (cube['zlevels'], cube['proj_info'], cube['resolution'])
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    e = CP.grid(150e3, 1e3)
    cspec = CP.Composite('ZH', e, e)
    op.load_model_ensemble([cube['data']] + [perturbed(cube['data'], 100 + m) for m in range(1, a.members)], *grid)
    spec = NB.Fractions(cspec, 'ZH', CP.from_db(THRESHOLDS_DBZ), [0])
    observed = np.array(op.simulate_rays_ensemble_composite(az, el, cspec, members=[1])['composite']['values']['ZH']['max'][0])
    kw = dict(connectivity=CONNECTIVITY, min_area=MIN_AREA, max_objects=MAX_OBJECTS)
    if a.worker in ('ens_match', 'ens_match_labels'):
        kw.update(match=True, max_pieces=MAX_PIECES)
    ospec = OB.Objects(spec, labels=a.worker not in ('ens_cells_bare', 'ens_match'), **kw)
    if a.worker == 'ens_host_match':
        def run():
            res = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed)
            res['composite']['objects'], res['n_pairs'] = host_match(OB, res['composite']['objects'], CONNECTIVITY)
            return res
    else:
        run = lambda: op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed)      # noqa: E731
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
    ob = w['objects']
    out = {'call': a.worker, 'n_rays': N_RAYS, 'n_gates': len(op.constants.RANGE_RADAR), 'steps': a.steps, 'members': a.members,
           'ms_per_call_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
           'max_checksum': float(np.nansum(w['values']['ZH']['max'], dtype=np.float64)),
           'sums_checksum': [int(np.array(w['fractions'][k]).sum(dtype=np.uint64)) for k in ('diff2', 'forecast2', 'observed2')],
           'cells_checksum': [int(np.array(ob[k]).sum(dtype=np.uint64)) for k in ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')],
           'n_objects_member_0': [int(x) for x in np.array(ob['n_objects'])[0]], 'n_objects_observed': [int(x) for x in np.array(ob['observed']['n_objects'])],
           'thresholds_dbz': THRESHOLDS_DBZ, 'terms': [CONNECTIVITY, MIN_AREA, MAX_OBJECTS, MAX_PIECES]}
    if 'pieces' in ob:
        pc = ob['pieces']
        out['match_checksum'] = [int(np.array(pc[k]).sum(dtype=np.uint64)) for k in ('n_pieces', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'forecast', 'observed')] \
            + [int(np.array(ob[k]).sum(dtype=np.uint64)) for k in ('covered', 'covered_observed')]
        out['n_pieces_member_0'] = [int(x) for x in np.array(pc['n_pieces'])[0]]
        out['n_pieces_max'] = int(np.array(pc['n_pieces']).max())
        out['n_pairs'] = int(res['n_pairs']) if 'n_pairs' in res else int(sum(OB.pairs(ob, b, t)['area'].size for b in range(a.members)
                                                                                for t in range(len(THRESHOLDS_DBZ))))
        size = lambda x: sum(size(v) for v in x.values()) if isinstance(x, dict) else int(np.asarray(x).nbytes)      # noqa: E731
        out['match_bytes'] = size(pc) + size(ob['covered']) + size(ob['covered_observed'])
    if a.worker != 'ens_host_match':
        out['bytes'] = handed_bytes({k: (v if k != 'objects' else {q: r for q, r in v.items() if q not in ('pieces', 'covered', 'covered_observed')})
                                     for k, v in w.items()})
    else:
        out['labels_bytes'] = int(np.array(ob['labels']).nbytes + np.array(ob['observed']['labels']).nbytes)
    print(json.dumps(out))
    op.close()


def driver(a):
    here = os.path.abspath(__file__)
    tags = list(WORKERS) + (['parent_ens_cells'] if a.parent_tree else [])
    if a.calls:
        tags = [t for t in a.calls.split(',') if t and t != 'none']           # (none: only --kernel-stats, with --update)
    runs = {t: [] for t in tags}
    common = ['--steps', str(a.steps), '--warmup', str(a.warmup), '--members', str(a.members)]
    for rep in range(a.repeat):
        for tag in tags:
            tree = os.path.abspath(a.parent_tree) if tag.startswith('parent_') else ROOT
            cmd = [sys.executable, here, '--worker', tag.replace('parent_', ''), '--tree', tree] + common
            r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.process_timeout)
            if r.returncode != 0:
                raise SystemExit('object_match_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            print('rep %d  %-17s %.4f ms per call (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_call_median'], rec['ms_min'], rec['ms_max']), flush=True)
    result = {'workload': 'bench.make_inputs(c2): %d rays x 500 gates, one lane, %d members; per-member ZH max maps on 300 x 300 cells of '
                          '1 km, thresholds %s dBZ, radius 0, observed = the map of member 1; cells: connectivity %d, min_area %d, '
                          '%d table rows, %d piece rows' % (N_RAYS, a.members, THRESHOLDS_DBZ, CONNECTIVITY, MIN_AREA, MAX_OBJECTS, MAX_PIECES),
              'method': 'blocking calls with page-locked outputs, %d steps after %d warm-up calls per process, %d fresh processes per '
                        'call, alternating' % (a.steps, a.warmup, a.repeat),
              'not_measured': 'several lanes in flight, device-resident outputs, a domain mask, other grids, connectivities, thresholds '
                              'and member counts, the single sweep, a volume, the largest grid, piece tables that overflow',
              'calls': {}}
    for tag, recs in runs.items():
        med = [r['ms_per_call_median'] for r in recs]
        c = {'ms_per_call_median_of_processes': float(np.median(med)), 'ms_per_call_medians': med,
             'spread': float((max(med) - min(med)) / np.median(med))}
        for k in ('max_checksum', 'members', 'sums_checksum', 'n_objects_member_0', 'n_objects_observed', 'cells_checksum', 'thresholds_dbz',
                  'terms', 'bytes', 'match_checksum', 'n_pieces_member_0', 'n_pieces_max', 'n_pairs', 'match_bytes', 'labels_bytes'):
            if k in recs[0]:
                c[k] = recs[0][k]
        result['calls'][tag] = c
    if a.update and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        old['calls'].update(result['calls'])
        old['method'] = result['method'] if old.get('method') == result['method'] else old.get('method', '') + '; ' + result['method']
        result = old
    calls = result['calls']
    ms = lambda tag: calls[tag]['ms_per_call_median_of_processes']       # noqa: E731
    if 'ens_match' in calls and 'ens_cells_bare' in calls:
        result['match_cost_ms'] = ms('ens_match') - ms('ens_cells_bare')
    if 'ens_match' in calls and 'ens_host_match' in calls:
        result['match_on_device_over_labels_and_host_match_ms'] = [ms('ens_match'), ms('ens_host_match')]
        result['match_equal'] = bool(calls['ens_match'].get('match_checksum') == calls['ens_host_match'].get('match_checksum')
                                     and calls['ens_match'].get('n_pairs') == calls['ens_host_match'].get('n_pairs'))
    if 'parent_ens_cells' in calls and 'ens_cells' in calls:
        cc, pc = calls['ens_cells'], calls['parent_ens_cells']
        margin = max(cc['spread'], pc['spread'])
        result['control_call_without_match'] = {'ens_cells_over_parent_ms': ms('ens_cells') / ms('parent_ens_cells'),
                                                'range_ms': [min(cc['ms_per_call_medians']), max(cc['ms_per_call_medians'])],
                                                'parent_range_ms': [min(pc['ms_per_call_medians']), max(pc['ms_per_call_medians'])],
                                                'margin_the_larger_spread': margin,
                                                'not_slower_within_the_margin': bool(ms('ens_cells') <= ms('parent_ens_cells') * (1.0 + margin)),
                                                'each_median_inside_the_others_range': inside(cc['ms_per_call_medians'], pc['ms_per_call_medians']),
                                                'checksums_equal': bool(pc.get('max_checksum') == cc.get('max_checksum')
                                                                        and pc.get('sums_checksum') == cc.get('sums_checksum')
                                                                        and pc.get('cells_checksum') == cc.get('cells_checksum'))}
    for item in a.kernel_stats or []:
        name, path = item.split('=', 1)
        tb = kernel_table(path)
        # (the profiler's database keeps the names as it finds them: plain, demangled, or mangled as _Z<length><name><arguments>)
        result.setdefault('kernels', {})[name] = {k: tb.get(k) or next((v for n, v in tb.items() if '_Z%d%s' % (len(k), k) in n
                                                                        or re.search(k + r'(?![A-Za-z0-9_])', n)), None) for k in KERNELS}
        result.setdefault('kernel_lists', {})[name] = {n: v['calls'] for n, v in sorted(tb.items())}
    lists = result.get('kernel_lists', {})
    if 'ens_cells' in lists and 'parent_ens_cells' in lists:
        result['control_kernel_list_equals_parent'] = lists['ens_cells'] == lists['parent_ens_cells']
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--track', action='store_true', help='the track of a series of scan times instead: profiles/object_track_profile.json')
    ap.add_argument('--times', type=int, default=12, help='with --track: the scan times of the series')
    ap.add_argument('--worker', choices=WORKERS + TRACK_WORKERS, default=None, help='one process of one call: prints one JSON line')
    ap.add_argument('--tree', default=ROOT, help='with --worker: the checkout whose package and bench inputs are used')
    ap.add_argument('--trace', action='store_true', help='with --worker: the warm-up calls alone, for rocprofv3 --kernel-trace')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--members', type=int, default=21, help='members of the ensemble')
    ap.add_argument('--repeat', type=int, default=3, help='fresh processes per call')
    ap.add_argument('--calls', default=None, help='the calls of this session of the driver, comma-separated (default: all that apply)')
    ap.add_argument('--update', action='store_true', help='join the calls of this session to those --out already holds')
    ap.add_argument('--process-timeout', type=float, default=400.0)
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--kernel-stats', action='append', default=None, metavar='NAME=FILE')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'object_track_profile.json' if a.track else 'object_match_profile.json')
    if a.track:
        (track_worker if a.worker else track_driver)(a)
    elif a.worker:
        worker(a)
    else:
        driver(a)


if __name__ == '__main__':
    main()
