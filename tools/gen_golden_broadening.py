#!/usr/bin/env python
"""tools/gen_golden_broadening.py -- TEST INFRASTRUCTURE ONLY.

Generates the broadening fixtures tests/golden/radial_d3_{turb,motion}*.npz and broaden_rows.npz by running the REFERENCE
itself (imported by path through oracle/ref_shim.py, as oracle/gen_golden.py does) on the seeded inputs of
tests/_broadening.py.  Runs only where the reference is mounted; the fixtures are data.

ONE emulation, recorded in every fixture (`config_rebound` = 1): the reference's spectral_width_turb / spectral_width_motion
read a module-level CONFIG of scatter/doppler_scatter.py that was bound at import time, when it was still None; the name
is rebound to the live configuration.  The arithmetic is the reference's.  The melting case also runs under
ref_shim.numpy1_linspace (`numpy1_linspace` = 1), as the d3_melt* goldens do.

The per-sub-beam intermediates (raw spectrum, the two widths, the switch, the broadened spectrum, the attenuation
per gate) are what the reference's
own functions returned while its get_radar_observables ran: they are recorded by wrappers around those functions.

usage: python tools/gen_golden_broadening.py [--out tests/golden] [--only NAME ...]
"""
import argparse
import copy
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden  # noqa: E402
import ref_shim  # noqa: E402
import _broadening as B  # noqa: E402

warnings.simplefilter('ignore')


class Recorder(object):
    """Wraps five functions of the reference's doppler_scatter module for the duration of one get_radar_observables."""
    NAMES = ('get_doppler_spectrum', 'spectral_width_turb', 'spectral_width_motion', 'broaden_spectrum', 'nan_cumsum')

    def __init__(self, ds):
        self.ds = ds
        self.subs = []

    def __enter__(self):
        self.real = {n: getattr(self.ds, n) for n in self.NAMES}

        def spectrum(*a, **k):
            out = self.real['get_doppler_spectrum'](*a, **k)
            self.subs.append({'raw': np.array(out, copy=True), 'on': 0})
            return out

        def turb(*a, **k):
            out = self.real['spectral_width_turb'](*a, **k)
            self.subs[-1]['w_turb'] = np.array(out, copy=True)
            return out

        def motion(*a, **k):
            out = self.real['spectral_width_motion'](*a, **k)
            self.subs[-1]['w_motion'] = np.array(out, copy=True)
            return out

        def broaden(spec, std):
            self.subs[-1]['w'] = np.array(std, copy=True)
            out = self.real['broaden_spectrum'](spec, std)
            self.subs[-1]['on'] = 1
            self.subs[-1]['broad'] = np.array(out, copy=True)
            return out

        def cumsum(x, *a, **k):
            # (the first call after a sub-beam's spectrum is the one of its attenuation, doppler_scatter.py:375)
            if self.subs and 'ah' not in self.subs[-1]:
                self.subs[-1]['ah'] = np.array(x, copy=True)
            return self.real['nan_cumsum'](x, *a, **k)
        for n, f in zip(self.NAMES, (spectrum, turb, motion, broaden, cumsum)):
            setattr(self.ds, n, f)
        return self

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(self.ds, n, f)


def gen_radial(name):
    from cosmo_pol_amd import synthetic
    from cosmo_pol.config import cfg
    from cosmo_pol.constants import global_constants as constants
    from cosmo_pol.interpolation import get_interpolated_radial
    from cosmo_pol.scatter import cut_at_sensitivity
    from cosmo_pol.scatter import doppler_scatter as ds
    from cosmo_pol_oracle.config import hydrometeor_list, make_config
    over, az, el, cube, two = B.case_inputs(name)
    conf = ref_shim.configure_reference(over)
    ds.CONFIG = cfg.CONFIG                       # the one emulation: the dead module-level name is made live
    scheme, freq = conf['microphysics']['scheme'], conf['radar']['frequency']
    hl = hydrometeor_list(make_config(over))
    luts = gen_golden.ref_luts({h: synthetic.make_lut(h, freq, scheme, **gen_golden.LUT_KW) for h in hl})
    order = list(gen_golden.ORDER_2MOM if two else gen_golden.ORDER) + (['EDR'] if 'EDR' in cube['data'] else [])
    dv = ref_shim.KeyListDict()
    for n in order:
        dv[n] = ref_shim.ModelVar(n, cube['data'][n].copy(), cube['zlevels'], cube['proj_info'], cube['resolution'])
    subs = get_interpolated_radial(dv, az, el, N=0)
    d = dict(azimuth=az, elevation=el, n_sub=len(subs), config_rebound=1)
    turb, motion = bool(conf['doppler']['turbulence_correction']), bool(conf['doppler']['motion_correction'])
    # ---- inputs: every sub-radial as the reference's interpolation left it (before its elevations are folded in place)
    for s, sb in enumerate(subs):
        for n in sb.values:
            d['sub%d_%s' % (s, n)] = np.asarray(sb.values[n]).copy()
        d['sub%d_mask' % s] = np.asarray(sb.mask).copy()
        d['sub%d_lats' % s] = np.asarray(sb.lats_profile).copy()
        d['sub%d_lons' % s] = np.asarray(sb.lons_profile).copy()
        d['sub%d_s' % s] = np.asarray(sb.dist_profile).copy()
        d['sub%d_h' % s] = np.asarray(sb.heights_profile).copy()
        d['sub%d_e' % s] = np.asarray(sb.elev_profile).copy()
        d['sub%d_has_melting' % s] = int(bool(getattr(sb, 'has_melting', False)))
    d['quad_w'] = np.array([float(sb.quad_weight) for sb in subs])
    d['quad_pts'] = np.array([sb.quad_pt for sb in subs], dtype=np.float64)
    with Recorder(ds) as rec:
        if name.endswith('melt'):
            with ref_shim.numpy1_linspace():
                obs = ds.get_radar_observables(subs, luts)
            d['numpy1_linspace'] = 1
        else:
            obs = ds.get_radar_observables(subs, luts)
    assert len(rec.subs) == len(subs)
    for s, r in enumerate(rec.subs):
        ng = r['raw'].shape[0]
        w = np.zeros(ng)                          # (doppler_scatter.py:361-366)
        if turb:
            w += r['w_turb']
        if motion:
            w += r['w_motion']
        if r['on']:
            assert np.array_equal(w, r['w'])
        d['sub%d_spec_raw' % s] = r['raw']
        d['sub%d_width' % s] = w
        d['sub%d_switch' % s] = r['on']
        d['sub%d_spec_broad' % s] = r['broad'] if r['on'] else r['raw']
        if conf['microphysics']['with_attenuation']:
            d['sub%d_ah' % s] = r['ah']           # the sub-beam's attenuation per gate, before its cumulative sum
    for n in obs.values:
        d['obs_' + n] = np.asarray(obs.values[n])
    d['obs_mask'] = obs.mask
    cut = cut_at_sensitivity([[copy.deepcopy(obs)]])[0][0]
    for n in cut.values:
        d['cutll_' + n] = np.asarray(cut.values[n])
    d['varray'] = np.asarray(constants.VARRAY, dtype=np.float64)
    d['range_radar'] = np.asarray(constants.RANGE_RADAR, dtype=np.float64)
    d['wavelength'] = float(constants.WAVELENGTH)
    on = [r['on'] for r in rec.subs]
    if name == 'd3_turb_masked':
        # the all-or-nothing switch pinned both ways on the reference's own sub-radials
        bad = [bool((~np.isfinite(d['sub%d_width' % s])).any()) for s in range(len(subs))]
        assert any(bad) and not all(bad), bad
        assert on == [int(not b) for b in bad], (on, bad)
    elif name in B.PLANTINGS:
        # bad values in the model data: one NaN width switches the broadening of a sub-beam off, under mask 0 as under a
        # mask born from the data; the conditions of tests/_broadening.coverage_failures against the clean twin's fixture
        bad = [bool((~np.isfinite(d['sub%d_width' % s])).any()) for s in range(len(subs))]
        assert on == [int(not b) for b in bad], (on, bad)
        clean = np.load(os.path.join(ROOT, 'tests', 'golden', 'radial_%s.npz' % B.CLEAN_TWIN[name]))
        unmet, counts = B.coverage_failures(name, d, clean)
        print('  coverage', counts)
        assert not unmet, (name, unmet)
    else:
        assert all(on), on
    sp = d['obs_DSPECTRUM']
    v_res = d['varray'][2] - d['varray'][1]
    print(name, 'n_sub', len(subs), 'switch', on, 'gates', sp.shape[0], 'bins', sp.shape[1], 'NaN gates', int(np.isnan(sp).all(1).sum()),
          'sigma/dv %.2f-%.2f' % tuple(np.nanpercentile(np.concatenate([d['sub%d_width' % s] for s in range(len(subs))]) / v_res, [0, 100])),
          'occupied bins', int((sp > 0).sum(1).min()), '-', int((sp > 0).sum(1).max()))
    return d


def gen_rows():
    from cosmo_pol.constants import global_constants as constants
    from cosmo_pol.scatter import doppler_scatter as ds
    d = dict(config_rebound=0)
    for rows, sig in B.function_rows():
        n_v = rows.shape[1]
        # broaden_spectrum takes its bin width from constants.VARRAY: a unit-spaced array of the row length makes std = sigma in bins
        saved = constants.VARRAY
        constants.VARRAY = np.arange(n_v, dtype=np.float64)
        try:
            out = ds.broaden_spectrum(rows.copy(), sig.copy())
        finally:
            constants.VARRAY = saved
        d['rows_%d' % n_v], d['sigma_%d' % n_v], d['out_%d' % n_v] = rows, sig, np.asarray(out)
        print('broaden_rows n_v', n_v, 'NaN rows', int(np.isnan(out).all(1).sum()), out.dtype)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    ap.add_argument('--only', nargs='*')
    a = ap.parse_args()
    ref_shim.load_reference()
    for name in B.CASES:
        if a.only and name not in a.only:
            continue
        np.savez_compressed(os.path.join(a.out, 'radial_%s.npz' % name), **gen_radial(name))
    if not a.only or 'broaden_rows' in a.only:
        np.savez_compressed(os.path.join(a.out, 'broaden_rows.npz'), **gen_rows())


if __name__ == '__main__':
    main()
