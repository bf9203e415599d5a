#!/usr/bin/env python
"""tools/terrain_shadow_profile.py -- what terrain shadowing costs, and that a call without it costs what it did.

Seeded inputs from bench.make_inputs: wall time per call around calls that end in a device synchronise, page-locked outputs, in
fresh processes that alternate:

  c2_off / c2_on / c2_on_vis   simulate_rays of the C2 sweep (360 x 500 gates, one sub-beam, at 1 degree) with both keys absent,
             with integration/terrain_shadow, and with integration/terrain_visibility beside it.  With shadowing the sweep loses
             the fused single-beam form (k_interp_classify / the presence words) and gains k_terrain_shadow;
  parent_c2  c2_off of --parent-tree DIR (a checkout of the parent commit with its library built): the control;
  c3_off / c3_on               the C3 volume (5 elevations x 360 x 500, melting layer and ice): five pinned sweeps on five lanes, one wait;
  c4_off / c4_on               the 7 x 7 C4 share of one of 8 GPUs (45 rays x 5 elevations, 49 sub-beams) as one launch sequence;
  bench / parent_bench         (--bench) `python bench.py --gpus 1 --steps 20 --warmup 5` of this tree and of DIR: the result line.

Kernel times and launch counts come from runs of their own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/terrain_shadow_profile.py --worker c2 --shadow 1 --vis 1 --trace
pass the kernel statistics files with --kernel-stats NAME=FILE to have every kernel's calls and times written into the JSON
(NAME = c2_off and parent_c2: the control "the kernel list and launch counts of a sweep without shadowing are the parent's").

THE TERRAIN.  The synthetic bench cube buries its radar: the site stands at 1000 m under a model topography of ~1.4 km, so gate 0
of every sub-beam is below the topography, the reference's gate-by-gate rule simulates the gates above it all the same, and with
shadowing the whole sweep is blocked -- the calls above then measure a sweep that scatters nothing.  The calls `*r_off`, `*r_on`,
`c2r_on_vis` (--terrain ridge) rebuild the cube's z-levels by make_cube's hybrid formula over a topography capped at 900 m with one
ridge (an arc 20 km from the radar, 2 km wide, crest 1950 m, azimuths 60 .. 120 degrees: the terrain of
tests/test_gpu_terrain_shadow.py at bench size): a sixth of the rays is blocked behind the ridge at the low elevations, the rest
is untouched -- the figure for what the feature costs a sweep that still has its gates.

NOT measured: several lanes in flight for the C2 sweep, device-resident outputs, the ensemble and timed forms, the column call,
the distributed path, other terrains (the share of gates behind a hit decides what the second half of the sequence saves).

  python tools/terrain_shadow_profile.py --repeat 3 --parent-tree DIR --bench --out profiles/terrain_shadow_profile.json
  python tools/terrain_shadow_profile.py --worker c2 --shadow 1            (one process, one JSON line)
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
ELEVATIONS = [0.5, 1.5, 3.0, 5.0, 8.0]           # bench.C4_ELEVATIONS
TAGS_RIDGE = {'c2r_off': ('c2', 0, 0), 'c2r_on': ('c2', 1, 0), 'c2r_on_vis': ('c2', 1, 1), 'c3r_off': ('c3', 0, 0), 'c3r_on': ('c3', 1, 0),
              'c4r_off': ('c4', 0, 0), 'c4r_on': ('c4', 1, 0)}
TAGS = {'c2_off': ('c2', 0, 0), 'c2_on': ('c2', 1, 0), 'c2_on_vis': ('c2', 1, 1), 'parent_c2': ('c2', 0, 0),
        'c3_off': ('c3', 0, 0), 'c3_on': ('c3', 1, 0), 'c4_off': ('c4', 0, 0), 'c4_on': ('c4', 1, 0)}


def ridge_cube(cube, site_rot=(-0.4725, -1.7207), model_top=22000.0, r_km=20.0, width_km=2.0, crest=1950.0, sector=(60.0, 120.0),
               base_cap=900.0):
    """The cube over a topography capped at `base_cap` with one ridge around the radar (rotated latitude / longitude `site_rot`,
    the bench site); z-levels by synthetic.make_cube's hybrid formula."""
    z = cube['zlevels']
    nz, ny, nx = z.shape
    eta = ((nz - np.arange(nz) - 0.5) / nz).astype(np.float64) ** 1.5
    e_last = float(np.float32(eta[-1]))
    topo = np.minimum((z[-1].astype(np.float64) - model_top * e_last) / (1.0 - e_last), base_cap)
    res = float(cube['resolution'][0])
    y0 = (site_rot[0] - cube['proj_info']['La1']) / res
    x0 = (site_rot[1] - cube['proj_info']['Lo1']) / res
    jy, jx = np.mgrid[0:ny, 0:nx]
    dy, dx = (jy - y0) * res * 111.2, (jx - x0) * res * 111.2
    r, az = np.hypot(dx, dy), np.degrees(np.arctan2(dx, dy)) % 360.0
    ridge = np.where((az >= sector[0]) & (az <= sector[1]), crest * np.exp(-((r - r_km) / width_km) ** 2 / 2.0), 0.0)
    topo = np.maximum(topo, ridge).astype(np.float32)
    znew = (topo[None] + (np.float32(model_top) - topo)[None] * eta.astype(np.float32)[:, None, None]).astype(np.float32)
    return dict(cube, zlevels=znew)


def worker(a):
    tree = os.path.abspath(a.tree)
    for p in (tree, os.path.join(tree, 'tools')):
        sys.path.insert(0, p)
    import bench
    from cosmo_pol_amd import RadarOperator
    conf, hyds, cube, luts = bench.make_inputs(a.worker)
    if a.terrain == 'ridge':
        cube = ridge_cube(cube)
    if a.shadow:
        conf['integration']['terrain_shadow'] = 1
    if a.vis:
        conf['integration']['terrain_visibility'] = 1
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar', lanes=5 if a.worker == 'c3' else 1)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    if a.worker == 'c2':
        az, el = np.arange(360.0), np.full(360, 1.0)
        run = lambda: [op.simulate_rays(az, el)]                                  # noqa: E731
    elif a.worker == 'c3':
        az = np.arange(360.0)
        els = [np.full(360, e) for e in ELEVATIONS]

        def run():
            res = [op.simulate_rays(az, els[k], pinned=True, lane=k) for k in range(5)]
            for k in range(5):
                op.wait(k)
            return res
    else:
        az = np.tile(np.arange(0.0, 360.0, 8.0), 5)                               # 45 rays per sweep: the share of one of 8 GPUs
        el = np.repeat(ELEVATIONS, 45)
        run = lambda: [op.simulate_rays(az, el)]                                  # noqa: E731
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
    zh = np.concatenate([np.asarray(r['ZH']) for r in res])
    out = {'call': a.worker, 'terrain': a.terrain, 'shadow': a.shadow, 'visibility': a.vis, 'n_rays': int(zh.shape[0]), 'n_gates': int(zh.shape[1]),
           'n_sub': int(res[0]['n_sub']), 'steps': a.steps, 'ms_per_call_median': float(np.median(t)), 'ms_min': float(np.min(t)),
           'ms_max': float(np.max(t)), 'finite_zh': int(np.isfinite(zh).sum()), 'zh_checksum': float(np.nansum(zh, dtype=np.float64)),
           'launch_forms': op._ctx.launch_forms()}
    if a.vis:
        vis = np.concatenate([np.asarray(r['visibility']) for r in res])
        out['visibility_bytes'] = int(vis.nbytes)
        out['gates_fully_blocked'], out['gates_partly_blocked'] = int((vis == 0).sum()), int(((vis > 0) & (vis < 1)).sum())
    print(json.dumps(out))
    op.close()


def driver(a):
    here = os.path.abspath(__file__)
    tags = (['c2_off', 'c2_on', 'c2_on_vis'] + (['parent_c2'] if a.parent_tree else []) + ['c3_off', 'c3_on', 'c4_off', 'c4_on']
            + list(TAGS_RIDGE))
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
            else:
                w, sh, vis = TAGS[tag] if tag in TAGS else TAGS_RIDGE[tag]
                steps = a.steps if w != 'c4' else max(3, a.steps // 4)
                cmd = [sys.executable, here, '--worker', w, '--shadow', str(sh), '--vis', str(vis), '--tree', tree,
                       '--terrain', 'ridge' if tag in TAGS_RIDGE else 'bench', '--steps', str(steps), '--warmup', str(a.warmup)]
            r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.process_timeout)
            if r.returncode != 0:
                raise SystemExit('terrain_shadow_profile: %s ended with %d:\n%s' % (tag, r.returncode, r.stdout[-3000:]))
            rec = last_json_line(r.stdout)
            runs[tag].append(rec)
            if tag.endswith('bench'):
                print('rep %d  %-12s value %.4e gates/s, %.4f ms per step' % (rep, tag, rec['value'], rec['ms_per_step']), flush=True)
            else:
                print('rep %d  %-12s %.4f ms per call (min %.4f, max %.4f)' % (rep, tag, rec['ms_per_call_median'], rec['ms_min'],
                                                                              rec['ms_max']), flush=True)
    result = {'workload': 'bench.make_inputs: c2 = 360 x 500 gates at 1 degree, one sub-beam; c3 = 5 elevations x 360 x 500, melting + ice, five '
                          'pinned sweeps on five lanes; c4 = 45 rays x 5 elevations, 7 x 7 sub-beams, one launch sequence',
              'method': 'wall time around calls that end in a device synchronise, page-locked outputs, %d steps (c4: a quarter) after %d '
                        'warm-up calls per process, %d fresh processes per call, alternating' % (a.steps, a.warmup, a.repeat),
              'not_measured': 'several lanes in flight for the C2 sweep, device-resident outputs, the ensemble and timed forms, the column '
                              'call, the distributed path, other terrains',
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
        for k in ('n_rays', 'n_gates', 'n_sub', 'finite_zh', 'zh_checksum', 'launch_forms', 'visibility_bytes', 'gates_fully_blocked',
                  'gates_partly_blocked'):
            if k in recs[0]:
                c[k] = recs[0][k]
        result['calls'][tag] = c
    if a.update and a.out and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        old['calls'].update(result['calls'])
        old['method'] = result['method'] if old.get('method') == result['method'] else old.get('method', '') + '; ' + result['method']
        for k in ('kernels', 'control_kernel_list'):
            if k in old:
                result[k] = old[k]
        result['calls'], result['method'] = old['calls'], old['method']
    calls = result['calls']
    ms = lambda tag: calls[tag]['ms_per_call_median_of_processes']       # noqa: E731
    for w in ('c2', 'c3', 'c4', 'c2r', 'c3r', 'c4r'):
        if w + '_off' in calls and w + '_on' in calls:
            result[w + '_on_over_off_ms'] = ms(w + '_on') / ms(w + '_off')
            result[w + '_on_minus_off_ms'] = ms(w + '_on') - ms(w + '_off')
    for w in ('c2', 'c2r'):
        if w + '_on_vis' in calls and w + '_on' in calls:
            result[w + '_visibility_cost_ms'] = ms(w + '_on_vis') - ms(w + '_on')
    if 'parent_c2' in calls and 'c2_off' in calls:
        cc, pc = calls['c2_off'], calls['parent_c2']
        result['control_c2'] = {'off_over_parent_ms': ms('c2_off') / ms('parent_c2'),
                                'range_ms': [min(cc['ms_per_call_medians']), max(cc['ms_per_call_medians'])],
                                'parent_range_ms': [min(pc['ms_per_call_medians']), max(pc['ms_per_call_medians'])],
                                'each_median_inside_the_others_range': inside(cc['ms_per_call_medians'], pc['ms_per_call_medians']),
                                'checksum_equal': bool(pc.get('zh_checksum') == cc.get('zh_checksum')),
                                'launch_forms_equal': bool(pc.get('launch_forms') == cc.get('launch_forms'))}
    if 'parent_bench' in calls and 'bench' in calls:
        b, pb = calls['bench'], calls['parent_bench']
        result['control_bench'] = {'value_over_parent': b['value_median'] / pb['value_median'],
                                   'range': [min(b['values']), max(b['values'])], 'parent_range': [min(pb['values']), max(pb['values'])],
                                   'each_median_inside_the_others_range': inside(b['values'], pb['values'])}
    for item in a.kernel_stats or []:
        name, path = item.split('=', 1)
        tb = kernel_table(path)
        result.setdefault('kernels', {})[name] = {k: {'calls': v['calls'], 'avg_us': v['avg_us'], 'min_us': v['min_us'], 'max_us': v['max_us']}
                                                  for k, v in sorted(tb.items())}
    ks = result.get('kernels', {})
    if 'c2_off' in ks and 'parent_c2' in ks:
        mine, theirs = ({k: v['calls'] for k, v in ks[n].items()} for n in ('c2_off', 'parent_c2'))
        result['control_kernel_list'] = {'kernels_and_launch_counts_equal': bool(mine == theirs), 'this_tree': mine, 'parent': theirs}
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', choices=('c2', 'c3', 'c4'), default=None, help='one process of one call: prints one JSON line')
    ap.add_argument('--shadow', type=int, default=0, help='with --worker: integration/terrain_shadow')
    ap.add_argument('--vis', type=int, default=0, help='with --worker: integration/terrain_visibility')
    ap.add_argument('--terrain', choices=('bench', 'ridge'), default='bench', help="with --worker: the cube's topography (see above)")
    ap.add_argument('--tree', default=ROOT, help='with --worker: the checkout whose package and bench inputs are used')
    ap.add_argument('--trace', action='store_true', help='with --worker: the warm-up calls alone, for rocprofv3 --kernel-trace')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
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
