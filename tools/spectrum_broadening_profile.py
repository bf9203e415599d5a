#!/usr/bin/env python
"""tools/spectrum_broadening_profile.py -- times Doppler scheme 3 with and without the spectrum broadening on a full sweep.

The `radial_d3_turb_fft256` configuration (tests/_broadening.py: 60 gates of 300 m, FFT_length 256, one sub-beam, rain / snow /
graupel / ice) widened to a PPI of --rays azimuths.  Wall time per sweep around blocking simulate_rays calls (each ends in a
device synchronise); kernel times come from running this script under `rocprofv3 --kernel-trace --stats -- python ...`.

usage: python tools/spectrum_broadening_profile.py --turb 1 --motion 1 [--rays 360] [--steps 30] [--warmup 5]
prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--turb', type=int, default=1)
    ap.add_argument('--motion', type=int, default=1)
    ap.add_argument('--rays', type=int, default=360)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    import _broadening as B
    import _cases
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_oracle import config as ocfg
    B.CASES['profile'] = ('d3_1mom_ice_sub', {'radar': {'FFT_length': 256}, 'integration': {'nh_GH': 1, 'nv_GH': 1},
                                              'doppler': {'turbulence_correction': a.turb, 'motion_correction': a.motion}}, None)
    over, az, el, cube, two = B.case_inputs('profile')
    conf = ocfg.make_config(over)
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme'])
            for h in ocfg.hydrometeor_list(conf)}
    op = RadarOperator(config=over, luts=luts, output_variables='only_radar')
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    azs, els = np.arange(a.rays) * (360.0 / a.rays), np.full(a.rays, el)
    for _ in range(a.warmup):
        res = op.simulate_rays(azs, els)
    t = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        res = op.simulate_rays(azs, els)
        t.append((time.perf_counter() - t0) * 1e3)
    sp = res['DSPECTRUM']
    print(json.dumps({'turb': a.turb, 'motion': a.motion, 'n_rays': a.rays, 'n_gates': sp.shape[1], 'n_vbins': sp.shape[2],
                      'steps': a.steps, 'ms_per_sweep_median': float(np.median(t)), 'ms_min': float(np.min(t)),
                      'ms_max': float(np.max(t)), 'nan_gates': int(np.isnan(res['RVEL']).sum()),
                      'spectrum_checksum': float(np.nansum(sp))}))
    op.close()


if __name__ == '__main__':
    main()
