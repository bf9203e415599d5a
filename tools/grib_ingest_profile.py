#!/usr/bin/env python
"""Wall time of RadarOperator.load_model_file at the bench cube's size (80 x 774 x 1158): the raw model output as an .npz
through the host path (model_io.derive in NumPy, one upload and one k_stage_variable launch per variable -- the code of
every release before the GRIB ingest, so the baseline) against the same fields as GRIB-1 at 16 bits through the device
ingest (packed octets over PCIe, k_grib_unpack, k_model_derive).

  python tools/grib_ingest_profile.py --write DIR            write DIR/lfff.grb, DIR/lfffc.grb, DIR/raw.npz (seeded)
  python tools/grib_ingest_profile.py DIR [--repeat 3]       alternating fresh processes per variant; one JSON line each
  python tools/grib_ingest_profile.py --run grib DIR         one measurement in this process (what the driver starts, and
                                                             what a `rocprofv3 --kernel-trace --stats` run wraps)
Variants: npz (host path), grib (device ingest).
--shape NZ NY NX shrinks the cube (a smoke run)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOUTH_POLE = (-43.0, 10.0)
VARIANTS = ('npz', 'grib')


def write_files(d, shape, seed=20261016):
    from cosmo_pol_amd import grib1, model_io
    nz, ny, nx = shape
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                          # noqa: E731
    hhl = f32(np.linspace(22000., 0., nz + 1)[:, None, None] + 400.0 * rng.random((1, ny, nx), dtype=np.float32))
    zf = 0.5 * (hhl[:-1] + hhl[1:])
    raw = {'T': f32(288.0 - 6.5e-3 * zf), 'P': f32(101325.0 * np.exp(-zf / 8000.0))}
    del zf
    raw['QV'] = f32(1e-3 + 4e-3 * rng.random(shape, dtype=np.float32))
    for k in ('QR', 'QC', 'QI', 'QS', 'QG'):
        raw[k] = f32(1e-3 * rng.random(shape, dtype=np.float32))
    for k in ('U', 'V'):
        raw[k] = f32(10.0 * rng.standard_normal(shape, dtype=np.float32))
    raw['W'] = f32(rng.standard_normal((nz + 1, ny, nx), dtype=np.float32))
    rlon, rlat = -6.8 + 0.01 * np.arange(nx), -4.4 + 0.01 * np.arange(ny)
    t0 = time.time()
    grib1.write_grib1(os.path.join(d, 'lfff.grb'), raw, rlon, rlat, SOUTH_POLE, n_bits=16)
    grib1.write_grib1(os.path.join(d, 'lfffc.grb'), {'HHL': hhl}, rlon, rlat, SOUTH_POLE, n_bits=16)
    t1 = time.time()
    # the .npz holds what the GRIB file decodes to: both variants stage the same cube
    g, c = grib1.Grib1File(os.path.join(d, 'lfff.grb')), grib1.Grib1File(os.path.join(d, 'lfffc.grb'))
    dec = {k: g.get(k) for k in raw}
    model_io.write_npz(os.path.join(d, 'raw.npz'), dec, hhl=c.get('HHL'), proj_info=g.proj_info())
    g.close()
    c.close()
    print(json.dumps({'wrote': d, 'shape': shape, 'grib_bytes': os.path.getsize(os.path.join(d, 'lfff.grb')),
                      'cfile_bytes': os.path.getsize(os.path.join(d, 'lfffc.grb')),
                      'npz_bytes': os.path.getsize(os.path.join(d, 'raw.npz')), 'write_grib_s': round(t1 - t0, 1)}))


def kernel_bytes(nz, ny, nx, n_raw_planes, packed_octets, n_vars):
    """What each kernel must move, from the shapes: (k_grib_unpack, k_model_derive) bytes."""
    ncell = ny * nx
    planes = 4 * ncell * n_raw_planes
    return packed_octets + planes, planes + 4 * ncell * nz * n_vars + 4 * ncell * nz + 8 * ncell


def run_one(variant, d):
    import bench
    from cosmo_pol_amd import RadarOperator, synthetic
    luts = synthetic.make_all_luts(('R', 'S', 'G'), 5.6, '1mom', n_e=8)
    op = RadarOperator(config=bench.bench_config(True), luts=luts, output_variables='only_radar')
    out = {'variant': variant}
    if variant == 'npz':
        files = (os.path.join(d, 'raw.npz'),)
    else:
        files = (os.path.join(d, 'lfff.grb'), os.path.join(d, 'lfffc.grb'))
        t0 = time.perf_counter()
        g, c = op._open_packed(*files)
        out['index_scan_ms'] = round(1e3 * (time.perf_counter() - t0), 2)
        out['packed_octets'] = int(sum(m['n_octets'] for s in (g, c) for lv in s.g.fields.values() for m in lv.values()))
        out['n_planes'] = int(sum(len(lv) for s in (g, c) for lv in s.g.fields.values()))
        g.close()
        c.close()
    for f in files:                                                          # the page cache holds the files, as after a model run
        with open(f, 'rb') as fh:
            while fh.read(1 << 26):
                pass
    t0 = time.perf_counter()
    op.load_model_file(*files)
    out['load_model_file_ms'] = round(1e3 * (time.perf_counter() - t0), 2)
    if variant != 'npz':
        assert op._packed is not None
        t = op._ctx.ingest_times()
        nz, (ny, nx) = op._packed['nz'], op._packed['g'].g.shape()
        ub, db = kernel_bytes(nz, ny, nx, out['n_planes'], out['packed_octets'], len(op._staged_vars))
        out.update({'upload_ms': round(t['upload_ms'], 2), 'k_grib_unpack_ms': round(t['unpack_ms'], 3),
                    'k_model_derive_ms': round(t['derive_ms'], 3), 'stage_call_ms': round(t['total_ms'], 2),
                    'upload_GBps': round(out['packed_octets'] / t['upload_ms'] / 1e6, 1),
                    'unpack_bytes': ub, 'unpack_TBps': round(ub / t['unpack_ms'] / 1e9, 2),
                    'derive_bytes': db, 'derive_TBps': round(db / t['derive_ms'] / 1e9, 2)})
    # one sweep, so that a wrong cube would show
    res = op.simulate_rays(np.arange(0.0, 360.0, 30.0), np.full(12, 2.0))
    out['finite_ZH'] = int(np.isfinite(res['ZH']).sum())
    out['ZH_checksum'] = float(np.nansum(res['ZH'].astype(np.float64)))
    op.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('dir')
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--run', choices=sorted(VARIANTS))
    ap.add_argument('--variants', nargs='+', default=list(VARIANTS), choices=sorted(VARIANTS))
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--shape', type=int, nargs=3, default=[80, 774, 1158])
    a = ap.parse_args()
    if a.write:
        return write_files(a.dir, tuple(a.shape))
    if a.run:
        return run_one(a.run, a.dir)
    for _ in range(a.repeat):                                                # alternating, a fresh process each
        for v in a.variants:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--run', v, a.dir], capture_output=True,
                               text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode                                          # (nothing more is started after a failure)
            print([l for l in r.stdout.splitlines() if l.startswith('{')][-1], flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
