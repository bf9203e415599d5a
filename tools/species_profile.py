#!/usr/bin/env python
"""What hydrometeor contributions cost: the 360 x 500 R+S+G sweep of bench.make_inputs('c2'), one lane,
page-locked host outputs, BLOCKING calls; needs a GPU.  Every figure comes from fresh processes, the kinds alternating, at
least three processes per figure: the median and the range of their per-call times.

  species        simulate_rays_species(az, el, Species(('ZH', 'ZDR', 'KDP'), dominant=True))
  plain_general  simulate_rays under CPOL_GATE1=0: the same launch sequence without the product (the difference is the product's cost)
  plain          simulate_rays in its default form (what a caller gives up by asking)
  host           the host alternative: a debug context's sz_integ pulled after simulate_rays, plus species.fields_of

A child (--child KIND) warms up, then times blocking calls for --window seconds and prints one JSON line: ms per call, the bytes
handed over per call, the launch forms.  `plain` and `plain_general` import nothing of the feature: with --control TREE the parent
process also runs them in TREE (a built checkout of another commit) alternately with this tree, and bench.py of both.
k_species alone comes from a run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/species_profile.py --child trace
pass its average with --kernel-us to have it written into the JSON (--child trace_plain: the plain call's 30 untimed calls, for the
kernel list and launch counts of a tree).

NOT measured: sub-beam volumes, other field sets, several lanes in flight, pinned (non-blocking) calls, device outputs.

  python tools/species_profile.py --out profiles/species_profile.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('species', 'plain_general', 'plain', 'host')
COORDS = ('lats', 'lons', 'dist', 'heights')          # cached per table set: not handed over again


def child(kind, window):
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('species_profile: needs a GPU')
    import bench
    from cosmo_pol_amd import RadarOperator
    conf, hyds, cube, luts = bench.make_inputs('c2')
    az, el = np.arange(360.0), np.full(360, 1.0)
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    ng = len(op.constants.RANGE_RADAR)
    if kind in ('species', 'trace'):
        from cosmo_pol_amd import species as SP
        spec = SP.Species(('ZH', 'ZDR', 'KDP'), dominant=True)

        def call():
            return op.simulate_rays_species(az, el, spec)
    elif kind == 'host':
        from cosmo_pol_amd import species as SP
        op._ctx.enable_debug()
        consts = SP.constants_of(float(op.constants.WAVELENGTH), float(op.config['radar']['K_squared']))
        n_hyd = len(op._staged_hydro)

        def call():
            res = op.simulate_rays(az, el)
            sz = op._ctx.debug_read('sz_integ', (360, ng, n_hyd, 12), np.float32)
            res['species'] = SP.fields_of(sz, np.array(res['ZH']), *consts)
            res['species']['sz'] = sz
            return res
    else:
        def call():
            return op.simulate_rays(az, el)
    for _ in range(3 if kind == 'host' else 30):
        res = call()
    if kind in ('trace', 'trace_plain'):          # (30 untimed calls, for rocprofv3 --kernel-trace: species / the plain call)
        op.close()
        return
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < window or n < 3:
        res = call()                                    # (blocking: the results are complete when it returns)
        n += 1
    ms = (time.perf_counter() - t0) / n * 1e3
    nbytes = sum(v.nbytes for k, v in res.items() if isinstance(v, np.ndarray) and k not in COORDS)
    sp_bytes = 0
    if 'species' in res:
        part = res['species']
        sp_bytes = sum(v.nbytes for k, v in part.items() if isinstance(v, np.ndarray) and (kind != 'host' or k == 'sz'))
    out = {'kind': kind, 'ms_per_call': ms, 'calls': n, 'bytes_per_call': nbytes + sp_bytes, 'species_bytes_per_call': sp_bytes,
           'launch_forms': {k: int(v) for k, v in op._ctx.launch_forms().items()}, 'n_gates': ng,
           'env_CPOL_GATE1': os.environ.get('CPOL_GATE1')}
    op.close()
    print('SPECIES_PROFILE ' + json.dumps(out, sort_keys=True), flush=True)


def spawn(tree, kind, window):
    env = dict(os.environ)
    env.pop('CPOL_GATE1', None)
    if kind == 'plain_general':
        env['CPOL_GATE1'] = '0'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'species_profile.py'), '--child', kind, '--window', str(window),
                        '--tree', tree], capture_output=True, text=True, env=env, timeout=600)
    if r.returncode != 0:
        raise SystemExit('child %s in %s failed (%d)\n%s\n%s' % (kind, tree, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    line = [l for l in r.stdout.splitlines() if l.startswith('SPECIES_PROFILE ')][-1]
    return json.loads(line[len('SPECIES_PROFILE '):])


def bench_once(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'],
                       capture_output=True, text=True, cwd=tree, timeout=900)
    if r.returncode != 0:
        raise SystemExit('bench.py in %s failed (%d)\n%s' % (tree, r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])


def summary(values):
    return {'median': float(np.median(values)), 'min': float(min(values)), 'max': float(max(values)), 'values': [float(v) for v in values]}


def main():
    global ROOT
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None)
    ap.add_argument('--tree', default=ROOT, help='(child) the checkout whose package is measured')
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--control', default=None, help='a built checkout of the commit to compare the plain call and bench.py with')
    ap.add_argument('--kernel-us', type=float, default=None, help="k_species' average from the rocprofv3 run")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        ROOT = os.path.abspath(args.tree)
        return child(args.child, args.window)
    if args.rounds < 3:
        raise SystemExit('at least three processes per figure')
    runs = {k: [] for k in KINDS}
    control = {'plain': [], 'plain_general': []}
    for rnd in range(args.rounds):
        for kind in KINDS:
            runs[kind].append(spawn(ROOT, kind, args.window))
            print(rnd, kind, '%.4f ms' % runs[kind][-1]['ms_per_call'], flush=True)
            if args.control and kind in control:
                control[kind].append(spawn(args.control, kind, args.window))
                print(rnd, 'control', kind, '%.4f ms' % control[kind][-1]['ms_per_call'], flush=True)
    result = {'sweep': '360 x 500 gates, R+S+G, one sub-beam (bench.make_inputs c2), one lane, page-locked outputs, blocking calls',
              'processes_per_figure': args.rounds, 'window_s': args.window,
              'not_measured': 'sub-beam volumes, other field sets, several lanes in flight, pinned calls, device outputs'}
    for kind in KINDS:
        rec = summary([r['ms_per_call'] for r in runs[kind]])
        rec.update({k: runs[kind][-1][k] for k in ('bytes_per_call', 'species_bytes_per_call', 'launch_forms', 'n_gates')})
        result[kind] = rec
    result['product_cost_ms'] = result['species']['median'] - result['plain_general']['median']
    result['given_up_ms'] = result['species']['median'] - result['plain']['median']
    if args.kernel_us is not None:
        result['k_species_us'] = args.kernel_us
    if args.control:
        ctl = {'tree': 'the parent commit'}
        for kind in control:
            ctl[kind] = summary([r['ms_per_call'] for r in control[kind]])
            ctl[kind]['launch_forms'] = control[kind][-1]['launch_forms']
            a, b = result[kind], ctl[kind]
            ctl[kind]['each_median_inside_the_others_range'] = bool(b['min'] <= a['median'] <= b['max'] and a['min'] <= b['median'] <= a['max'])
        here, there = [], []
        for rnd in range(args.rounds):
            here.append(bench_once(ROOT))
            there.append(bench_once(args.control))
            print(rnd, 'bench', here[-1].get('value'), there[-1].get('value'), flush=True)
        key = 'value' if 'value' in here[0] else sorted(k for k, v in here[0].items() if isinstance(v, (int, float)))[0]
        a, b = summary([r[key] for r in here]), summary([r[key] for r in there])
        ctl['bench'] = {'figure': key, 'unit': here[0].get('unit'), 'this': a, 'control': b,
                        'each_median_inside_the_others_range': bool(b['min'] <= a['median'] <= b['max'] and a['min'] <= b['median'] <= a['max'])}
        result['control'] = ctl
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
