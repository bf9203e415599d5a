#!/usr/bin/env python
"""tools/objects_profile.py -- the object cells of scored composites on the device against labelling on the host.

The conditions of tools/fractions_profile.py: seeded inputs from bench.make_inputs('c2'), the 360 x 500 bench sweep, one lane, an
ensemble of --members states (the cube and seeded perturbations, form 'shared'); per-member ZH 'max' maps on the 300 x 300 grid of
1 km cells at three thresholds (18, 30, 40 dBZ), scored at radius 0 against the map of member 1; cells under 8-connectivity,
min_area 4, 1024 table rows.  Wall time per call around BLOCKING calls with page-locked outputs (each ends in a device
synchronise), in fresh processes that alternate:

  ens_cells        simulate_rays_ensemble_composite_fss with an objects.Objects: maps, scores, cells and label maps from the device;
  ens_cells_bare   the same without the label maps;
  ens_fss          the same call with a plain Fractions: scores only;
  ens_host         ens_fss, then the cells on the host: scipy.ndimage.label plus the attributes where SciPy is installed, else
                   objects.cells: what the device call replaces;
  parent_ens_fss   ens_fss of --parent-tree DIR (a checkout of the parent commit with its library built): the control for "a scored
                   call without the cells did not get slower";
  bench / parent_bench   (--bench) `python bench.py --gpus 1 --steps 20 --warmup 5` of this tree and of DIR: the result line.

Kernel times come from a run of its own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/objects_profile.py --worker ens_cells --trace
pass the kernel statistics file with --kernel-stats NAME=FILE to have the figures of the k_obj_* kernels written into the JSON.

With --sums ("exact sums") the calls are those of the exact sums, written to profiles/object_sums_profile.json:

  ens_sums_bare        scores, cells and the exact sums (volume, moments, field sums) from the device, WITHOUT the label maps;
  ens_cells_host_sums  ens_cells (with the label maps), then the three sums per object with np.bincount(weights=) over the label and
                       value maps on the host: what the sums on the device replace;
  ens_fss, parent_ens_fss, bench, parent_bench   the controls, as above.

Each record carries the bytes of the arrays handed over.  The kernel lists of the control (ens_fss of this tree and of the parent)
come from --kernel-stats ens_fss=FILE and --kernel-stats parent_ens_fss=FILE of runs of their own.

NOT measured: several lanes in flight, device-resident outputs, a domain mask, other grids, connectivities, thresholds and member
counts, the single sweep, a volume, the largest grid.

  python tools/objects_profile.py --repeat 3 --out profiles/objects_profile.json
  python tools/objects_profile.py --worker ens_cells            (one process, one JSON line)
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = 360
THRESHOLDS_DBZ = [18.0, 30.0, 40.0]
CONNECTIVITY, MIN_AREA, MAX_OBJECTS = 8, 4, 1024
WORKERS = ('ens_cells', 'ens_cells_bare', 'ens_fss', 'ens_host')
SUMS_WORKERS = ('ens_sums_bare', 'ens_cells_host_sums', 'ens_fss')
KERNELS = ('k_obj_runs', 'k_obj_merge', 'k_obj_flatten', 'k_obj_area', 'k_obj_count', 'k_obj_number', 'k_obj_attr', 'k_obj_decode', 'k_obj_sums', 'k_obj_sums_finish',
           'k_frac_rows', 'k_frac_cols', 'k_frac_score', 'k_comp_finish')


def host_cells(OB, spec, maps, observed):
    """The cells on the host: SciPy's labelling with the rule's attributes where it is installed, else the rule itself."""
    try:
        from scipy import ndimage
    except ImportError:
        return OB.cells(spec, maps, observed), 'objects.cells'
    F, O, m, o = OB.binary_maps(spec.fractions, maps, observed)
    element = np.ones((3, 3), dtype=int) if spec.connectivity == 8 else None
    n_blocks, n_thr = F.shape[:2]
    n = np.zeros((n_blocks + 1, n_thr), np.uint32)
    table = np.zeros((n_blocks + 1, n_thr, spec.max_objects, OB.WORDS), np.uint32)
    labels = np.zeros((n_blocks + 1, n_thr) + o.shape, np.int32)
    for s in range(n_blocks + 1):
        for t in range(n_thr):
            lab, count = ndimage.label(F[s, t] if s < n_blocks else O[t], structure=element)
            area = np.bincount(lab.reshape(-1), minlength=count + 1)
            keep = area >= spec.min_area
            keep[0] = False
            lab = np.where(keep, np.cumsum(keep), 0).astype(np.int32)[lab]
            n[s, t], labels[s, t] = int(keep.sum()), lab
            table[s, t] = OB._table(lab, int(keep.sum()), m[s] if s < n_blocks else o, spec.max_objects)
    return OB.result(spec, n, table, labels), 'scipy.ndimage.label'


def host_sums(ob, maps, observed):
    """The three float sums per object on the host from the label maps: np.bincount(weights=), float64 in the order of the cells (not
    reproducible from one NumPy build to the next; what a user did before the exact sums)."""
    labels = np.concatenate([np.array(ob['labels']), np.array(ob['observed']['labels'])[None]])
    values = np.concatenate([np.asarray(maps), np.asarray(observed)[None]]).astype(np.float64)
    n_src, n_thr, n_y, n_x = labels.shape
    yy, xx = np.indices((n_y, n_x))
    out = np.zeros((n_src, n_thr, MAX_OBJECTS + 1, 3))
    for s in range(n_src):
        v = np.nan_to_num(values[s], nan=0.0).reshape(-1)
        for t in range(n_thr):
            lab = np.minimum(labels[s, t].reshape(-1), MAX_OBJECTS + 1)
            for j, w in enumerate((v, v * xx.reshape(-1), v * yy.reshape(-1))):
                out[s, t, :, j] = np.bincount(lab, weights=w, minlength=MAX_OBJECTS + 2)[1:MAX_OBJECTS + 2]
    return out[:, :, :MAX_OBJECTS]


def handed_bytes(w):
    """The bytes of the arrays a scored call hands over: the maps, the scores and the cells' arrays."""
    def size(x):
        if isinstance(x, dict):
            return sum(size(v) for v in x.values())
        return int(np.asarray(x).nbytes) if hasattr(x, 'dtype') else 0
    ob = w.get('objects', {})
    own = {k: v for k, v in ob.items() if k not in ('thresholds', 'weight')}
    return {'maps': size(w['values']) + size(w['count']), 'scores': size({k: w['fractions'][k] for k in ('diff2', 'forecast2', 'observed2',
            'n_forecast', 'n_observed', 'n_domain')}), 'cells': size({k: v for k, v in own.items() if k != 'labels' and k != 'observed'})
            + size({k: v for k, v in own.get('observed', {}).items() if k != 'labels'}),
            'labels': size(own.get('labels', 0)) + size(own.get('observed', {}).get('labels', 0))}


def worker(a):
    tree = os.path.abspath(a.tree)
    for p in (tree, os.path.join(tree, 'tools')):
        sys.path.insert(0, p)
    import bench
    from timed_profile import perturbed
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_amd import composite as CP
    from cosmo_pol_amd import neighbourhood as NB
    conf, hyds, cube, luts = bench.make_inputs('c2')
    az, el = np.arange(float(N_RAYS)), np.full(N_RAYS, 1.0)
    grid = (cube['zlevels'], cube['proj_info'], cube['resolution'])
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    e = CP.grid(150e3, 1e3)
    cspec = CP.Composite('ZH', e, e)
    op.load_model_ensemble([cube['data']] + [perturbed(cube['data'], 100 + m) for m in range(1, a.members)], *grid)
    spec = NB.Fractions(cspec, 'ZH', CP.from_db(THRESHOLDS_DBZ), [0])
    # the observed map: member 1's own (another state of the same model), made once, outside the timed calls
    observed = np.array(op.simulate_rays_ensemble_composite(az, el, cspec, members=[1])['composite']['values']['ZH']['max'][0])
    how = 'device'
    if a.worker == 'ens_fss':
        run = lambda: op.simulate_rays_ensemble_composite_fss(az, el, spec, observed)
    else:
        from cosmo_pol_amd import objects as OB
        if a.worker == 'ens_sums_bare':
            ospec = OB.Objects(spec, connectivity=CONNECTIVITY, min_area=MIN_AREA, max_objects=MAX_OBJECTS, labels=False, sums=True)
        else:
            ospec = OB.Objects(spec, connectivity=CONNECTIVITY, min_area=MIN_AREA, max_objects=MAX_OBJECTS, labels=a.worker != 'ens_cells_bare')
        if a.worker == 'ens_cells_host_sums':
            def run():
                res = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed)
                res['host_sums'], res['how'] = host_sums(res['composite']['objects'], res['composite']['values']['ZH']['max'], observed), 'np.bincount(weights=)'
                return res
        elif a.worker == 'ens_host':
            def run():
                res = op.simulate_rays_ensemble_composite_fss(az, el, spec, observed)
                res['composite']['objects'], res['how'] = host_cells(OB, ospec, res['composite']['values']['ZH']['max'], observed)
                return res
        else:
            run = lambda: op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed)
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
    out = {'call': a.worker, 'n_rays': N_RAYS, 'n_gates': len(op.constants.RANGE_RADAR), 'steps': a.steps, 'members': a.members,
           'ms_per_call_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
           'max_checksum': float(np.nansum(w['values']['ZH']['max'], dtype=np.float64)),
           'sums_checksum': [int(np.array(w['fractions'][k]).sum(dtype=np.uint64)) for k in ('diff2', 'forecast2', 'observed2')]}
    out['bytes'] = handed_bytes(w)
    if 'objects' in w:
        ob = w['objects']
        if 'volume' in ob:
            # (the bits of the exact sums: equal in every process and on every run)
            out['exact_sums_checksum'] = [int(np.bitwise_xor.reduce(np.ascontiguousarray(np.array(ob[k])).view(np.uint64).reshape(-1)))
                                          for k in ('volume', 'moment_x', 'moment_y')]
            out['volume_member_0_first'] = [float(x) for x in np.array(ob['volume'])[0, :, 0]]
            out['field_volume_member_0'] = float(np.array(ob['field']['volume'])[0])
        if 'host_sums' in res:
            out['host_volume_member_0_first'] = [float(x) for x in res['host_sums'][0, :, 0, 0]]
        out['how'] = res.get('how', how) if isinstance(res, dict) else how
        out['n_objects_member_0'] = [int(x) for x in np.array(ob['n_objects'])[0]]
        out['n_objects_observed'] = [int(x) for x in np.array(ob['observed']['n_objects'])]
        out['largest_area'] = int(np.array(ob['area']).max())
        out['cells_checksum'] = [int(np.array(ob[k]).sum(dtype=np.uint64)) for k in ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')]
        out['thresholds_dbz'], out['terms'] = THRESHOLDS_DBZ, [CONNECTIVITY, MIN_AREA, MAX_OBJECTS]
    print(json.dumps(out))
    op.close()


def driver(a):
    here = os.path.abspath(__file__)
    tags = list(SUMS_WORKERS if a.sums else WORKERS)
    if a.parent_tree:
        tags.append('parent_ens_fss')
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
                raise SystemExit('objects_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            if tag.endswith('bench'):
                print('rep %d  %-15s value %.4e gates/s, %.4f ms per step' % (rep, tag, rec['value'], rec['ms_per_step']), flush=True)
            else:
                print('rep %d  %-15s %.4f ms per call (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_call_median'], rec['ms_min'],
                                                                               rec['ms_max']), flush=True)
    result = {'workload': 'bench.make_inputs(c2): %d rays x 500 gates, one lane, %d members; per-member ZH max maps on 300 x 300 cells of '
                          '1 km, thresholds %s dBZ, radius 0, observed = the map of member 1; cells: connectivity %d, min_area %d, '
                          '%d table rows' % (N_RAYS, a.members, THRESHOLDS_DBZ, CONNECTIVITY, MIN_AREA, MAX_OBJECTS),
              'method': 'blocking calls with page-locked outputs, %d steps after %d warm-up calls per process, %d fresh processes per '
                        'call, alternating' % (a.steps, a.warmup, a.repeat),
              'not_measured': 'several lanes in flight, device-resident outputs, a domain mask, other grids, connectivities, thresholds '
                              'and member counts, the single sweep, a volume, the largest grid',
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
        for k in ('max_checksum', 'members', 'sums_checksum', 'how', 'n_objects_member_0', 'n_objects_observed', 'largest_area',
                  'cells_checksum', 'thresholds_dbz', 'terms', 'bytes', 'exact_sums_checksum', 'volume_member_0_first',
                  'field_volume_member_0', 'host_volume_member_0_first'):
            if k in recs[0]:
                c[k] = recs[0][k]
        if 'exact_sums_checksum' in recs[0]:
            c['exact_sums_equal_in_every_process'] = all(r['exact_sums_checksum'] == recs[0]['exact_sums_checksum'] for r in recs)
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
    if all(t in calls for t in WORKERS):
        result['cells_cost_ms'] = ms('ens_cells') - ms('ens_fss')
        result['cells_bare_cost_ms'] = ms('ens_cells_bare') - ms('ens_fss')
        result['host_cells_cost_ms'] = ms('ens_host') - ms('ens_fss')
        result['cells_equal'] = bool(calls['ens_cells'].get('cells_checksum') == calls['ens_host'].get('cells_checksum')
                                     and calls['ens_cells'].get('sums_checksum') == calls['ens_fss'].get('sums_checksum'))
    if all(t in calls for t in SUMS_WORKERS[:2]):
        result['sums_on_device_over_labels_and_host_sums_ms'] = [ms('ens_sums_bare'), ms('ens_cells_host_sums')]
        result['cells_equal'] = bool(calls['ens_sums_bare'].get('cells_checksum') == calls['ens_cells_host_sums'].get('cells_checksum'))
    if 'parent_ens_fss' in calls and 'ens_fss' in calls:
        cc, pc = calls['ens_fss'], calls['parent_ens_fss']
        result['control_scored_call'] = {'ens_fss_over_parent_ms': ms('ens_fss') / ms('parent_ens_fss'),
                                         'range_ms': [min(cc['ms_per_call_medians']), max(cc['ms_per_call_medians'])],
                                         'parent_range_ms': [min(pc['ms_per_call_medians']), max(pc['ms_per_call_medians'])],
                                         'each_median_inside_the_others_range': inside(cc['ms_per_call_medians'], pc['ms_per_call_medians']),
                                         'checksums_equal': bool(pc.get('max_checksum') == cc.get('max_checksum')
                                                                 and pc.get('sums_checksum') == cc.get('sums_checksum'))}
    if 'parent_bench' in calls and 'bench' in calls:
        b, pb = calls['bench'], calls['parent_bench']
        result['control_bench'] = {'value_over_parent': b['value_median'] / pb['value_median'],
                                   'range': [min(b['values']), max(b['values'])], 'parent_range': [min(pb['values']), max(pb['values'])],
                                   'each_median_inside_the_others_range': inside(b['values'], pb['values'])}
    for item in a.kernel_stats or []:
        name, path = item.split('=', 1)
        tb = kernel_table(path)
        # (the profiler's database keeps the mangled names: the kernel whose name holds k)
        result.setdefault('kernels', {})[name] = {k: tb.get(k) or next((v for n, v in tb.items() if re.search(k + r'(?![A-Za-z0-9_])', n)), None)
                                                  for k in KERNELS}
        result.setdefault('kernel_lists', {})[name] = {n: v['calls'] for n, v in sorted(tb.items())}
    lists = result.get('kernel_lists', {})
    if 'ens_fss' in lists and 'parent_ens_fss' in lists:
        result['control_kernel_list_equals_parent'] = lists['ens_fss'] == lists['parent_ens_fss']
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', choices=WORKERS + SUMS_WORKERS[:2], default=None, help='one process of one call: prints one JSON line')
    ap.add_argument('--tree', default=ROOT, help='with --worker: the checkout whose package and bench inputs are used')
    ap.add_argument('--trace', action='store_true', help='with --worker: the warm-up calls alone, for rocprofv3 --kernel-trace')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--members', type=int, default=21, help='members of the ensemble')
    ap.add_argument('--repeat', type=int, default=3, help='fresh processes per call')
    ap.add_argument('--calls', default=None, help='the calls of this session of the driver, comma-separated (default: all that apply)')
    ap.add_argument('--update', action='store_true', help='join the calls of this session to those --out already holds')
    ap.add_argument('--sums', action='store_true', help='the calls of the exact sums instead (profiles/object_sums_profile.json)')
    ap.add_argument('--bench', action='store_true', help="bench.py's result line too (of the parent tree as well)")
    ap.add_argument('--process-timeout', type=float, default=400.0)
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--kernel-stats', action='append', default=None, metavar='NAME=FILE')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.sums and not a.out:
        a.out = os.path.join(ROOT, 'profiles', 'object_sums_profile.json')
    if a.worker:
        worker(a)
    else:
        driver(a)


if __name__ == '__main__':
    main()
