#!/usr/bin/env python
"""oracle/gen_golden.py -- TEST INFRASTRUCTURE ONLY.

Generates tests/golden/*.npz by running the REFERENCE itself (imported by path
from /root/reference through oracle/ref_shim.py) on seeded synthetic inputs.
Runs only in the build container (the GPU box has no /root/reference); the
resulting fixtures are data (inputs + expected outputs) and are committed
together with this script.

Geodesy note: the reference's two third-party geodesy calls (pyproj, pycosmo)
are bound by the shim to the oracle's own implementation, so everything
downstream of them is pinned, the geodesy itself is not.

usage: python oracle/gen_golden.py [--out tests/golden]
"""
import argparse
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_shim  # noqa: E402

warnings.simplefilter('ignore')

CUBE_KW = dict(nz=30, res=0.02, half_width_deg=0.55, seed=7)
ORDER = ['U', 'V', 'W', 'QR_v', 'QS_v', 'QG_v', 'QI_v', 'RHO', 'T']
ORDER_2MOM = ORDER + ['QH_v', 'QNH_v', 'QNR_v', 'QNS_v', 'QNG_v', 'QNI_v']


def ref_luts(luts):
    from cosmo_pol.lookup.lut import Lookup_table
    out = {}
    for h, s in luts.items():
        L = Lookup_table()
        L.axes, L.axes_names = s.axes, s.axes_names
        L.axes_limits, L.axes_step = s.axes_limits, s.axes_step
        L.value_table = s.value_table
        out[h] = L
    return out


def gen_gate_kernel(out):
    """get_all_radar_pts of the compiled reference C on random + adversarial
    small cubes (bit-exact fixture)."""
    interp = ref_shim._loaded['interp_module']
    rng = np.random.default_rng(11)
    nz, ny, nx = 12, 9, 10
    topo = rng.uniform(0, 800, size=(ny, nx)).astype(np.float32)
    eta = ((nz - np.arange(nz) - 0.5) / nz) ** 1.3
    zl = (topo[None] + (9000 - topo)[None] * eta[:, None, None]).astype(np.float32)
    data = rng.normal(size=(nz, ny, nx)).astype(np.float32)
    llc = np.array([-1.0, 2.0], dtype=np.float32)        # (lon, lat)
    res = np.array([0.02, 0.025], dtype=np.float32)
    n = 400
    rlat = rng.uniform(llc[1] + 0.001, llc[1] + res[1] * (ny - 1) - 0.001, n)
    rlon = rng.uniform(llc[0] + 0.001, llc[0] + res[0] * (nx - 1) - 0.001, n)
    h = rng.uniform(-200, 10500, n)
    # adversarial gates: exactly on grid nodes / levels / top / lowest level
    rlat[:8] = llc[1] + res[1] * np.arange(8)
    rlon[:8] = llc[0] + res[0] * np.arange(8)
    coords = np.stack([rlat, rlon], axis=1).astype(np.float32)
    h = h.astype(np.float32)
    for k in range(8):                                    # exactly on a level of cell (k,k)
        h[k] = zl[k + 2, k, k]
    h[8] = zl[0, 3, 3]
    coords[8] = [llc[1] + res[1] * 3, llc[0] + res[0] * 3]
    h[9] = zl[-1, 4, 4]
    coords[9] = [llc[1] + res[1] * 4, llc[0] + res[0] * 4]
    h[10] = np.float32(zl[-1, 5, 5] + 0.5)               # between ground level and level nz-2
    coords[10] = [llc[1] + res[1] * 5.5, llc[0] + res[0] * 5.5]
    vals = interp.get_all_radar_pts(n, coords, h, data, zl, llc, res)[1]
    out['gate_kernel'] = dict(coords=coords, heights=h, data=data, zlevels=zl, llc=llc, res=res,
                              expected=vals)
    # binary_search known answers
    arr = np.array([50., 40., 30., 20., 10., 5.], dtype=np.float32)
    keys = np.array([60., 50., 45., 40., 25., 10., 7., 5., 4.], dtype=np.float32)
    out['gate_kernel']['bs_arr'] = arr
    out['gate_kernel']['bs_keys'] = keys
    out['gate_kernel']['bs_expected'] = np.array([interp.binary_search(arr, k) for k in keys],
                                                 dtype=np.int32)


def gen_trajectory(out):
    from cosmo_pol.interpolation.atm_refraction import _ref_4_3
    from cosmo_pol.utilities import get_earth_radius
    ref_shim.configure_reference({'radar': {'coords': [46.0, 7.0, 500], 'frequency': 5.6,
                                            'range': 150000, 'radial_resolution': 300}})
    from cosmo_pol.constants import global_constants as gc
    rr = gc.RANGE_RADAR
    d = dict(range_vec=rr, earth_radius_7=np.float64(get_earth_radius(7.0)),
             wavelength=np.float64(gc.WAVELENGTH))
    elevs = np.array([0.0, 0.5, 1.0, 3.0, 10.0, 45.0, 89.0, 95.0, -0.3])
    d['elevations'] = elevs
    for i, e in enumerate(elevs):
        s, h, el = _ref_4_3(rr, e, [46.0, 7.0, 500])
        d['s_%d' % i], d['h_%d' % i], d['e_%d' % i] = s, h, el
    out['trajectory'] = d


def refractivity_field(cube):
    """Synthetic refractivity N (N-units) for the small test cube."""
    z = cube['zlevels'].astype(np.float64)
    return (315.0 * np.exp(-z / 7350.0) * (1 + 0.02 * np.sin(z / 900.0))).astype(np.float32)


# NB refraction scheme 2 (_ref_ODE, atm_refraction.py:79-148) cannot be pinned by the
# reference here: under NumPy >= 1.24 its _deriv_z returns a ragged [scalar, 1-element
# array] list and scipy.integrate.odeint raises ValueError (an ordinary Python error of
# the reference itself).  The oracle restatement (cosmo_pol_oracle/refraction_ode.py)
# returns scalars; product and oracle are compared with each other in tests/.


def gen_quadrature(out):
    """Weights / kept sub-beams, recovered from get_interpolated_radial's
    output on a trivial cube."""
    from cosmo_pol_amd import synthetic
    from cosmo_pol.interpolation import get_interpolated_radial
    cube = synthetic.small_test_cube(nz=6, res=0.05, half_width_deg=0.3, seed=3)
    d = {}
    cases = [(1, 1, 1.0), (3, 3, 1.0), (7, 7, 1.0), (3, 9, 1.0), (3, 9, 0.999), (5, 5, 0.9)]
    for ci, (nh, nv, thr) in enumerate(cases):
        ref_shim.configure_reference({
            'radar': {'coords': [46.5, 7.5, 1000], 'frequency': 5.6, 'range': 5000,
                      'radial_resolution': 500, '3dB_beamwidth': 1.3},
            'integration': {'nh_GH': nh, 'nv_GH': nv, 'weight_threshold': thr}})
        dv = ref_shim.KeyListDict()
        dv['T'] = ref_shim.ModelVar('T', cube['data']['T'], cube['zlevels'], cube['proj_info'],
                                    cube['resolution'])
        subs = get_interpolated_radial(dv, 10.0, 5.0, N=0)
        d['case_%d' % ci] = np.array([nh, nv, thr])
        d['pts_%d' % ci] = np.array([s.quad_pt for s in subs])
        d['w_%d' % ci] = np.array([s.quad_weight for s in subs])
    out['quadrature'] = d


def gen_psd(out):
    from cosmo_pol.hydrometeors import create_hydrometeor
    rng = np.random.default_rng(5)
    d = {}
    n = 12
    QM = (10 ** rng.uniform(-6, -2.5, n)).astype(np.float32)
    T_liq = rng.uniform(265, 300, n).astype(np.float32)
    T_sol = rng.uniform(210, 274, n).astype(np.float32)
    fw = rng.uniform(0.01, 0.98, n)
    d.update(QM=QM, T_liq=T_liq, T_sol=T_sol, fw=fw)
    ksel = np.arange(0, 1024, 37)
    d['ksel'] = ksel
    axes = {}
    from cosmo_pol_amd import synthetic
    for h in ['R', 'S', 'G', 'I']:
        axes[h] = synthetic.make_lut(h, 5.6, '1mom', n_e=2, n_t=2).axes[2]
    for h in ['R', 'S', 'G', 'I', 'mS', 'mG']:
        hy = create_hydrometeor(h, '1mom')
        if h in axes:
            hy.d_min, hy.d_max = axes[h][0], axes[h][-1]
        if h in ('R', 'G'):
            hy.set_psd(QM)
        elif h in ('S', 'I'):
            hy.set_psd(T_sol, QM)
        elif h == 'mS':
            hy.set_psd(T_sol + 30, QM.astype(np.float64), fw)
        else:
            hy.set_psd(QM.astype(np.float64), fw)
        if h in ('mS', 'mG'):
            from cosmo_pol.utilities import vlinspace
            D = vlinspace(hy.d_min, hy.d_max, 1024)
            N = hy.get_N(D)
            d[h + '_dmin'], d[h + '_dmax'] = hy.d_min, hy.d_max
            d[h + '_prop'] = hy.prop_factor
            d[h + '_N'] = N[:, ksel]
            d[h + '_Nsum'] = N.sum(axis=1)
            v, nn = hy.integrate_V()
            d[h + '_vint'], d[h + '_nint'] = v, nn
        else:
            D = axes[h]
            N = hy.get_N(D)
            d[h + '_lambda'] = np.asarray(hy.lambda_)
            d[h + '_N0'] = np.asarray(hy.N0)
            d[h + '_N'] = N[:, ksel]
            d[h + '_Nsum'] = N.sum(axis=1)
            d[h + '_Ndtype'] = str(N.dtype)
            v, nn = hy.integrate_V()
            d[h + '_vint'], d[h + '_nint'] = np.asarray(v), np.asarray(nn)
    # 2-moment
    QN = {}
    for h in ['R', 'S', 'G', 'H', 'I']:
        hy = create_hydrometeor(h, '2mom')
        xm = np.sqrt(hy.x_min * hy.x_max)
        qn = (QM / (xm * 10 ** rng.uniform(-1.5, 1.5, n))).astype(np.float32)
        QN[h] = qn
        d['2m_QN_' + h] = qn
        ax = synthetic.make_lut(h, 13.6, '2mom', n_e=2, n_t=2).axes[2]
        hy.d_min, hy.d_max = ax[0], ax[-1]
        hy.set_psd(qn, QM)
        N = hy.get_N(ax)
        d['2m_%s_lambda' % h] = np.asarray(hy.lambda_)
        d['2m_%s_N0' % h] = np.asarray(hy.N0)
        d['2m_%s_N' % h] = N[:, ksel]
        d['2m_%s_Nsum' % h] = N.sum(axis=1)
    out['psd'] = d


def gen_pol(out):
    from cosmo_pol.scatter.doppler_scatter import get_pol_from_sz
    ref_shim.configure_reference({'radar': {'coords': [46.0, 7.0, 500], 'frequency': 5.6,
                                            'range': 150000, 'radial_resolution': 300}})
    rng = np.random.default_rng(9)
    base = np.array([1, -1, 1, 2, 3, -1, 1, 2, .5, .1, .7, .2])
    sz = (base[None] * 1e-3 * (1 + 0.3 * rng.normal(size=(40, 12)))).astype(np.float32)
    sz[5] = np.nan
    names = ['ZH', 'ZV', 'ZDR', 'RHOHV', 'KDP', 'AH', 'AV', 'DELTA_HV']
    res = get_pol_from_sz(sz, 0.93)
    d = dict(sz=sz)
    for n, r in zip(names, res):
        d[n] = np.asarray(r)
    out['pol'] = d


RADIAL_CASES = {
    # name: (config overrides, azimuth, elevation, hydrometeors kept in the cube, 2mom)
    'c1_rain_rhi': ({'radar': {'range': 30000, 'radial_resolution': 300},
                     'microphysics': {'with_ice_crystals': 0, 'with_melting': 0},
                     'integration': {'nh_GH': 1, 'nv_GH': 1}}, 45.0, 3.0, ('R',), False),
    'c2_rsg': ({'radar': {'range': 45000, 'radial_resolution': 300},
                'microphysics': {'with_ice_crystals': 0, 'with_melting': 0},
                'integration': {'nh_GH': 1, 'nv_GH': 1}}, 200.0, 4.0, ('R', 'S', 'G'), False),
    'c3_melt_ice': ({'radar': {'range': 45000, 'radial_resolution': 300},
                     'microphysics': {'with_ice_crystals': 1, 'with_melting': 1},
                     'integration': {'nh_GH': 1, 'nv_GH': 1}}, 120.0, 5.0,
                    ('R', 'S', 'G', 'I'), False),
    'c4_subbeams': ({'radar': {'range': 36000, 'radial_resolution': 600},
                     'microphysics': {'with_ice_crystals': 1, 'with_melting': 1},
                     'integration': {'nh_GH': 3, 'nv_GH': 5, 'weight_threshold': 0.999}},
                    300.0, 6.0, ('R', 'S', 'G', 'I'), False),
    'c2_noatt_hi_elev': ({'radar': {'range': 20000, 'radial_resolution': 250},
                          'microphysics': {'with_ice_crystals': 0, 'with_melting': 0,
                                           'with_attenuation': 0},
                          'integration': {'nh_GH': 1, 'nv_GH': 3}}, 10.0, 88.0,
                         ('R', 'S', 'G'), False),
    'c3_dop2': ({'radar': {'range': 36000, 'radial_resolution': 400},
                 'microphysics': {'with_ice_crystals': 1, 'with_melting': 1},
                 'doppler': {'scheme': 2},
                 'integration': {'nh_GH': 3, 'nv_GH': 1}}, 150.0, 4.5,
                ('R', 'S', 'G', 'I'), False),
    'c5_2mom': ({'radar': {'range': 30000, 'radial_resolution': 300, 'frequency': 13.6},
                 'microphysics': {'scheme': '2mom', 'with_ice_crystals': 1, 'with_melting': 0},
                 'integration': {'nh_GH': 1, 'nv_GH': 1}}, 75.0, 8.0, ('R', 'S', 'G', 'I'), True),
}

ANTENNA_CSV = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'antenna_diagram.csv')

# antenna quadratures other than scheme 1
RADIAL_CASES.update({
    'q_ml': ({'radar': {'range': 36000, 'radial_resolution': 400},
              'microphysics': {'with_ice_crystals': 0, 'with_melting': 1},
              'integration': {'scheme': 'ml', 'nh_GH': 1, 'nv_GH': 1}}, 120.0, 5.0,
             ('R', 'S', 'G'), False),
    'q_ml_thr': ({'radar': {'range': 30000, 'radial_resolution': 500},
                  'microphysics': {'with_ice_crystals': 1, 'with_melting': 1},
                  'integration': {'scheme': 'ml', 'nh_GH': 3, 'nv_GH': 1,
                                  'weight_threshold': 0.9999}}, 40.0, 3.0,
                 ('R', 'S', 'G', 'I'), False),
    'q_legendre': ({'radar': {'range': 30000, 'radial_resolution': 500},
                    'microphysics': {'with_ice_crystals': 0, 'with_melting': 0},
                    'integration': {'scheme': 3, 'nh_GH': 3, 'nv_GH': 3,
                                    'antenna_diagram': ANTENNA_CSV}}, 200.0, 4.0,
                   ('R', 'S', 'G'), False),
    'q_multigauss': ({'radar': {'range': 30000, 'radial_resolution': 500},
                      'microphysics': {'with_ice_crystals': 0, 'with_melting': 0},
                      'integration': {'scheme': 2, 'nr_GH': 3, 'na_GL': 3, 'weight_threshold': 0.99,
                                      'antenna_params': [[0.0, 0.0, 0.42], [-25.0, 1.8, 0.3],
                                                         [-32.0, 3.2, 0.4]]}}, 200.0, 4.0,
                     ('R', 'S', 'G'), False),
})

# Doppler scheme 3 (full spectrum, doppler_c.c); FFT_length 64 keeps the fixtures small
RADIAL_CASES.update({
    'd3_rsg': ({'radar': {'range': 24000, 'radial_resolution': 400, 'FFT_length': 64},
                'microphysics': {'with_ice_crystals': 0, 'with_melting': 0},
                'doppler': {'scheme': 3},
                'integration': {'nh_GH': 1, 'nv_GH': 1}}, 200.0, 4.0, ('R', 'S', 'G'), False),
    'd3_2mom_sub': ({'radar': {'range': 24000, 'radial_resolution': 600, 'frequency': 13.6,
                               'FFT_length': 32, 'PRI': 300},
                     'microphysics': {'scheme': '2mom', 'with_ice_crystals': 1, 'with_melting': 0,
                                      'with_attenuation': 0},
                     'doppler': {'scheme': 3},
                     'integration': {'nh_GH': 3, 'nv_GH': 1}}, 75.0, 8.0, ('R', 'S', 'G', 'I'), True),
})

# further combinations pinned by the reference itself
RADIAL_CASES.update({
    # (35 deg elevation: the fall-speed spread projects onto several velocity bins per gate)
    'd3_1mom_ice_sub': ({'radar': {'range': 18000, 'radial_resolution': 300, 'FFT_length': 32},
                         'microphysics': {'with_ice_crystals': 1, 'with_melting': 0},
                         'doppler': {'scheme': 3},
                         'integration': {'nh_GH': 3, 'nv_GH': 1}}, 120.0, 35.0, ('R', 'S', 'G', 'I'), False),
    'q_ml_dop2': ({'radar': {'range': 30000, 'radial_resolution': 500},
                   'microphysics': {'with_ice_crystals': 1, 'with_melting': 1},
                   'doppler': {'scheme': 2},
                   'integration': {'scheme': 'ml', 'nh_GH': 1, 'nv_GH': 1}}, 300.0, 6.0,
                  ('R', 'S', 'G', 'I'), False),
    'c5_2mom_dop2_sub': ({'radar': {'range': 24000, 'radial_resolution': 400, 'frequency': 13.6},
                          'microphysics': {'scheme': '2mom', 'with_ice_crystals': 1, 'with_melting': 0},
                          'doppler': {'scheme': 2},
                          'integration': {'nh_GH': 3, 'nv_GH': 3, 'weight_threshold': 0.999}}, 75.0, 8.0,
                         ('R', 'S', 'G', 'I'), True),
})

# BASELINE configs 4 and 5 at golden size: the full 7 x 7 Gauss-Hermite antenna quadrature
# (49 sub-beams, none dropped) over melting + ice, and the Ka-band (35.6 GHz, GPM-DPR KaPR,
# constants/global_constants.py:152-159) half of the dual-frequency 2-moment case
RADIAL_CASES.update({
    'c4_7x7': ({'radar': {'range': 36000, 'radial_resolution': 600},
                'microphysics': {'with_ice_crystals': 1, 'with_melting': 1},
                'integration': {'nh_GH': 7, 'nv_GH': 7, 'weight_threshold': 1.}},
               300.0, 6.0, ('R', 'S', 'G', 'I'), False),
    'c5_ka_2mom': ({'radar': {'range': 30000, 'radial_resolution': 250, 'frequency': 35.6,
                              '3dB_beamwidth': 0.5},
                    'microphysics': {'scheme': '2mom', 'with_ice_crystals': 1, 'with_melting': 0},
                    'integration': {'nh_GH': 1, 'nv_GH': 3}}, 75.0, 8.0, ('R', 'S', 'G', 'I'), True),
})

# Doppler scheme 3 WITH the melting scheme (round 6): the fall speed of a melting species is inverted
# through an interpolator rebuilt at every gate (set_psd clears it, hydrometeors.py:1426,1474; get_D_from_V :480-500).
# Every sub-beam of these radials crosses the melting layer: the reference drops mS / mG from a sub-beam without melting
# with `dict.keys().remove`, which raises under Python 3 (doppler_scatter.py:343-349).
RADIAL_CASES.update({
    # (30 / 40 deg elevation: the fall-speed spread of the melting particles projects onto several velocity bins per gate)
    'd3_melt': ({'radar': {'range': 9000, 'radial_resolution': 100, 'FFT_length': 64},
                 'microphysics': {'with_ice_crystals': 0, 'with_melting': 1},
                 'doppler': {'scheme': 3},
                 'integration': {'nh_GH': 1, 'nv_GH': 1}}, 120.0, 30.0, ('R', 'S', 'G'), False),
    'd3_melt_ice_sub': ({'radar': {'range': 7500, 'radial_resolution': 150, 'FFT_length': 32},
                         'microphysics': {'with_ice_crystals': 1, 'with_melting': 1},
                         'doppler': {'scheme': 3},
                         'integration': {'nh_GH': 3, 'nv_GH': 1}}, 300.0, 40.0, ('R', 'S', 'G', 'I'), False),
})

# ---- bad model values (NaN, the reference's own -9999 sentinel, negative or off-table values) ----
# A bad-value case is an existing case's configuration plus a deterministic planting applied to the synthetic cube.  One
# planting is (variable, value, r_lo, r_hi): every level of the grid columns whose distance from the centre of the cube --
# the radar site -- lies in [r_lo, r_hi) grid cells takes `value`; 'neg' negates what is there.  Rings, so that every
# azimuth and every sub-beam of a radial crosses them.  (One cell of the test cube is ~2.2 km.)
PLANTINGS = {
    # data-born masks (interpolation.py:398-411) under melting + ice: NaN / -9999 in variable 0, NaN in W (RVEL alone)
    'bad_c3_masks': ('c3_melt_ice', [('U', np.nan, 3.0, 5.0), ('U', -9999.0, 8.0, 12.5), ('W', np.nan, 14.0, 16.0)]),
    # mask 0, bad values: NaN in a mass density / T / RHO, negative mass density, T off both T axes (rain below and above
    # 262-314 K near the radar, snow below and above 200-276 K farther out)
    'bad_c3_values': ('c3_melt_ice', [('T', 150.0, 0.0, 1.5), ('T', 330.0, 2.5, 3.5), ('QR_v', np.nan, 4.5, 5.5),
                                      ('QS_v', 'neg', 8.0, 9.5), ('T', np.nan, 11.0, 12.0), ('T', 150.0, 13.5, 14.5),
                                      ('T', 330.0, 15.5, 16.5), ('RHO', np.nan, 17.5, 18.5)]),
    # sub-beams: both data-born masks, a NaN and a negative mass density seen by 3 x 5 sub-beams at different ranges
    'bad_c4_sub15': ('c4_subbeams', [('U', np.nan, 3.0, 4.5), ('QR_v', np.nan, 5.0, 6.5), ('U', -9999.0, 7.5, 15.0),
                                        ('QG_v', 'neg', 15.0, 17.0)]),
    # scheme 'ml' with melting: negative rain, wet fractions below the first and above the last node of the wc axis (rain /
    # snow + graupel of 1e-8 / 1e-9 kg m-3 against ~1e-3 of the partner), a NaN partner of the melting scheme
    'bad_q_ml': ('q_ml', [('QR_v', 'neg', 0.0, 1.5), ('QS_v', 1e-9, 3.0, 5.0), ('QG_v', 1e-9, 3.0, 5.0),
                          ('QR_v', 1e-8, 6.0, 7.5), ('QG_v', np.nan, 8.5, 9.5), ('U', np.nan, 11.0, 12.5)]),
    # 2-moment: QN zero, negative and NaN under a positive Q; a NaN mass density
    'bad_c5_2mom': ('c5_2mom', [('QNR_v', 0.0, 0.5, 2.8), ('QNR_v', 'neg', 3.5, 4.5), ('QNS_v', 0.0, 5.0, 7.3),
                                ('QNS_v', 'neg', 7.6, 8.4), ('QNG_v', np.nan, 8.8, 9.4), ('QS_v', np.nan, 9.8, 10.4),
                                ('QNI_v', np.nan, 11.5, 12.5)]),
    # Doppler spectrum with sub-beams (35 deg: ~0.11 cells per gate, 6.7 cells in all): NaN in W and in U
    'bad_d3_ice_sub': ('d3_1mom_ice_sub', [('W', np.nan, 2.4, 3.0), ('U', np.nan, 6.0, 7.5)]),
}
BAD_VALUE_CASES = list(PLANTINGS) + ['bad_hi_elev_fold']

for _name, (_base, _p) in PLANTINGS.items():
    RADIAL_CASES[_name] = RADIAL_CASES[_base]
# clean data, 89.6 deg: the upper vertical quadrature node looks beyond the zenith, its elevation is folded to 180 - e
# (doppler_scatter.py:173-176)
RADIAL_CASES['bad_hi_elev_fold'] = (
    {'radar': {'range': 20000, 'radial_resolution': 250},
     'microphysics': {'with_ice_crystals': 0, 'with_melting': 0, 'with_attenuation': 0},
     'integration': {'nh_GH': 1, 'nv_GH': 3}}, 10.0, 89.6, ('R', 'S', 'G'), False)


# what each bad-value case is there for: effect -> counted by coverage_counts() from the fixture alone, at least
# MIN_EFFECT_GATES gates each (and, every case, at least a third of the gates with a finite ZH)
MIN_EFFECT_GATES = 5
MIN_COUNT = {'spectrum_rows_kept': 20, 'spectrum_bins_kept': 40}          # effects with a minimum of their own
COVERAGE = {
    'bad_c3_masks': ['mask_m1_data', 'mask_p1_data', 'edge_m9999', 'rvel_nan_W'],
    'bad_c3_values': ['nan_QR_v', 'neg_QS_v', 'nan_T', 'nan_RHO', 'mask0_nan_ZH', 't_below_axes', 't_above_axes'],
    'bad_c4_sub15': ['mask_m1_data', 'mask_p1_data', 'mask_m1_two_subbeams', 'mask_p1_two_subbeams', 'edge_m9999',
                        'nan_QR_v', 'neg_QG_v'],
    'bad_q_ml': ['mask_m1_data', 'mask_m1_two_subbeams', 'neg_QR_v', 'nan_QG_v', 'mask0_nan_ZH', 'wc_first_bin',
                 'wc_below_axis', 'wc_last_bin'],
    'bad_c5_2mom': ['zero_QNR_v', 'neg_QNR_v', 'zero_QNS_v', 'neg_QNS_v', 'nan_QNG_v', 'nan_QNI_v', 'nan_QS_v',
                    'mask0_nan_ZH'],
    'bad_d3_ice_sub': ['mask_m1_data', 'mask_m1_two_subbeams', 'rvel_nan_W', 'spectrum_rows_kept',
                       'spectrum_bins_kept', 'spectrum_rows_lost'],
    'bad_hi_elev_fold': ['elev_above_90'],
}


def coverage_counts(d):
    """Gates of a bad-value fixture (the arrays of its .npz) that show each effect.  A data-born mask counts only where
    the reference's run on the UNPLANTED cube (clean_*) has mask 0: geometry cannot stand in for it."""
    with np.errstate(invalid='ignore'):
        zh = np.asarray(d['obs_ZH'])
        fin = np.isfinite(zh)
        m, mc = np.asarray(d['obs_mask']), np.asarray(d['clean_obs_mask'])
        sm, smc = np.asarray(d['sub_mask_all']), np.asarray(d['clean_sub_mask_all'])
        c0 = np.asarray(d['subc_mask']) == 0                  # the central sub-beam
        out = {'finite_ZH': int(fin.sum()), 'n_gates': int(zh.size),
               'mask_m1_data': int(((m == -1) & (mc == 0)).sum()),
               'mask_p1_data': int(((m == 1) & (mc == 0)).sum()),
               'mask0_nan_ZH': int(((m == 0) & ~fin & np.isfinite(d['clean_obs_ZH'])).sum()),
               'edge_m9999': int((c0 & (np.asarray(d['subc_U']) < -100.)).sum()),
               'rvel_nan_W': int((fin & c0 & np.isnan(d['subc_W']) & np.isnan(d['obs_RVEL'])
                                  & np.isfinite(d['clean_obs_RVEL'])).sum()),
               't_below_axes': int((fin & (np.asarray(d['subc_T']) < 200.)).sum()),
               't_above_axes': int((fin & (np.asarray(d['subc_T']) > 314.)).sum())}
        # the second best sub-beam: >= MIN_EFFECT_GATES there means more than one sub-beam crosses the planting
        for tag, val in (('m1', -1), ('p1', 1)):
            per_sub = np.sort(((sm == val) & (smc == 0)).sum(axis=1))
            out['mask_%s_two_subbeams' % tag] = int(per_sub[-2]) if per_sub.size > 1 else 0
        for k in d.keys() if hasattr(d, 'keys') else d.files:
            if k.startswith('subc_') and k not in ('subc_mask', 'subc_lats', 'subc_lons', 'subc_s', 'subc_h', 'subc_e'):
                v, a = k[5:], np.asarray(d[k])
                out['nan_' + v] = int((c0 & np.isnan(a)).sum())
                out['neg_' + v] = int((c0 & (a < 0)).sum())
                if v.startswith('QN'):
                    out['zero_' + v] = int((c0 & (a == 0) & (np.asarray(d['subc_Q' + v[2:]]) > 0)).sum())
        for h in ('mS', 'mG'):
            if 'subc_fwet_' + h in d:
                fw, q = np.asarray(d['subc_fwet_' + h]), np.asarray(d['subc_Q%s_v' % h])
                # (the wc axis of the melting tables: linspace(1e-3, 0.999, 100), bin = floor, clipped: lut.py:336-341)
                b = np.floor((fw - 1e-3) / (0.998 / 99))
                out['wc_first_bin'] = out.get('wc_first_bin', 0) + int((fin & (q > 0) & (b <= 0)).sum())
                out['wc_below_axis'] = out.get('wc_below_axis', 0) + int((fin & (q > 0) & (b < 0)).sum())
                out['wc_last_bin'] = out.get('wc_last_bin', 0) + int((fin & (q > 0) & (b >= 99)).sum())
        e_all = np.asarray(d['sub_e_all'])
        out['elev_above_90'] = int(((e_all > 90.) & (sm == 0)).sum(axis=1).max())
        if 'obs_DSPECTRUM' in d:
            sp, spc = np.asarray(d['obs_DSPECTRUM']), np.asarray(d['clean_obs_DSPECTRUM'])
            row = lambda a: np.isfinite(a).all(axis=1) & (a != 0).any(axis=1)
            out['spectrum_rows_kept'] = int(row(sp).sum())
            out['spectrum_bins_kept'] = int((np.isfinite(sp) & (sp != 0)).sum())
            out['spectrum_rows_lost'] = int((row(spc) & ~row(sp)).sum())
    return out


def coverage_failures(name, d):
    c = coverage_counts(d)
    bad = ['%s: %d < %d' % (k, c.get(k, 0), MIN_COUNT.get(k, MIN_EFFECT_GATES)) for k in COVERAGE[name]
           if c.get(k, 0) < MIN_COUNT.get(k, MIN_EFFECT_GATES)]
    if 3 * c['finite_ZH'] < c['n_gates']:
        bad.append('finite ZH at %d of %d gates' % (c['finite_ZH'], c['n_gates']))
    return bad, c


def plant_bad_values(cube, plantings):
    """Applies `plantings` (PLANTINGS) to the data of a synthetic cube, in place."""
    any_var = next(iter(cube['data'].values()))
    ny, nx = any_var.shape[1:]
    yy, xx = np.meshgrid(np.arange(ny) - (ny - 1) / 2., np.arange(nx) - (nx - 1) / 2., indexing='ij')
    r = np.hypot(yy, xx)
    for var, value, r_lo, r_hi in plantings:
        sel = (r >= r_lo) & (r < r_hi)
        a = cube['data'][var]
        if isinstance(value, str):
            assert value == 'neg'
            a[:, sel] = -a[:, sel]
        else:
            a[:, sel] = np.float32(value)
    return cube


LUT_KW = dict(seed=20260301, n_e=8, n_t=None)


def write_antenna_csv(path=ANTENNA_CSV):
    """Synthetic one-way antenna diagram (angle in deg, power in dB): Gaussian main
    lobe of 1 deg beamwidth plus two side lobes; a data fixture for schemes 2 / 3."""
    ang = np.round(np.arange(-5.0, 5.0 + 1e-9, 0.1), 1)
    sig = 1.0 / (2 * np.sqrt(2 * np.log(2)))
    p = (np.exp(-ang ** 2 / (2 * sig ** 2)) + 10 ** -2.6 * np.exp(-(np.abs(ang) - 1.9) ** 2 / (2 * 0.25 ** 2))
         + 10 ** -3.3 * np.exp(-(np.abs(ang) - 3.4) ** 2 / (2 * 0.35 ** 2)) + 1e-5)
    np.savetxt(path, np.column_stack([ang, 10 * np.log10(p)]), delimiter=',', fmt='%.6f')


def radial_case_inputs(name, clean=False):
    """Deterministic inputs of an end-to-end radial case (shared with
    tests/).  clean: a bad-value case without its planting."""
    from cosmo_pol_amd import synthetic
    over, az, el, hyds, two = RADIAL_CASES[name]
    base = {'radar': {'coords': [46.5, 7.5, 1000], 'frequency': 5.6, '3dB_beamwidth': 1.,
                      'K_squared': 0.93, 'type': 'ground', 'sensitivity': [-5, 10000]},
            'doppler': {'scheme': 1}}
    for sec, dd in over.items():
        base.setdefault(sec, {}).update(dd)
    cube = synthetic.small_test_cube(hydrometeors=hyds, two_moment=two, **CUBE_KW)
    if name in PLANTINGS and not clean:
        plant_bad_values(cube, PLANTINGS[name][1])
    return base, az, el, cube, two


def gen_radials(out, only_cases=None):
    from cosmo_pol_amd import synthetic
    from cosmo_pol.interpolation import get_interpolated_radial, integrate_radials
    from cosmo_pol.scatter import get_radar_observables
    from cosmo_pol_oracle.config import hydrometeor_list, make_config
    lut_cache = {}
    if not os.path.exists(ANTENNA_CSV):
        write_antenna_csv()
    for name in RADIAL_CASES:
        if only_cases and name not in only_cases:
            continue
        over, az, el, cube, two = radial_case_inputs(name)
        conf = ref_shim.configure_reference(over)
        scheme = conf['microphysics']['scheme']
        freq = conf['radar']['frequency']
        hl = hydrometeor_list(make_config(over))
        key = (scheme, freq)
        lut_cache.setdefault(key, {})
        for h in hl:
            if h not in lut_cache[key]:
                lut_cache[key][h] = synthetic.make_lut(h, freq, scheme, **LUT_KW)
        luts = ref_luts({h: lut_cache[key][h] for h in hl})
        def interpolate(cube):
            dv = ref_shim.KeyListDict()
            for n in (ORDER_2MOM if two else ORDER):
                dv[n] = ref_shim.ModelVar(n, cube['data'][n].copy(), cube['zlevels'],
                                          cube['proj_info'], cube['resolution'])
            return get_interpolated_radial(dv, az, el, N=0)
        subs = interpolate(cube)
        d = dict(azimuth=az, elevation=el, n_sub=len(subs))
        if name in BAD_VALUE_CASES:
            # every sub-beam's mask and elevation (before get_radar_observables folds it in place), and the reference on
            # the UNPLANTED cube: what coverage_counts() needs
            d['sub_mask_all'] = np.array([sb.mask for sb in subs])
            d['sub_e_all'] = np.array([sb.elev_profile for sb in subs])
            csubs = interpolate(radial_case_inputs(name, clean=True)[3])
            d['clean_sub_mask_all'] = np.array([sb.mask for sb in csubs])
            cobs = get_radar_observables(csubs, luts)
            d['clean_obs_mask'] = cobs.mask
            for n in ('ZH', 'RVEL', 'DSPECTRUM'):
                if n in cobs.values:
                    d['clean_obs_' + n] = np.asarray(cobs.values[n])
        ng = len(subs[0].dist_profile)
        d['quad_w'] = np.array([np.broadcast_to(sb.quad_weight, (ng,)) for sb in subs])
        d['quad_pts'] = np.array([sb.quad_pt for sb in subs], dtype=np.float64)
        c = subs[int(len(subs) / 2)]
        # interpolated model variables of the central + first sub-beam
        for tag, sb in (('c', c), ('f', subs[0])):
            for n in sb.values:
                d['sub%s_%s' % (tag, n)] = np.asarray(sb.values[n]).copy()
            d['sub%s_mask' % tag] = sb.mask.copy()
            d['sub%s_lats' % tag] = np.asarray(sb.lats_profile)
            d['sub%s_lons' % tag] = np.asarray(sb.lons_profile)
            d['sub%s_s' % tag] = sb.dist_profile.copy()
            d['sub%s_h' % tag] = sb.heights_profile.copy()
            d['sub%s_e' % tag] = sb.elev_profile.copy()
        integ = integrate_radials(subs)
        for n in integ.values:
            d['model_' + n] = np.asarray(integ.values[n])
        d['model_mask'] = integ.mask
        n_valid = {}
        for h in hl:
            n_valid[h] = int(sum(np.sum(np.asarray(s.values['Q' + h + '_v']) > 0) for s in subs
                                 if not (h in ('mS', 'mG') and not s.has_melting)))
        if name.startswith('d3_melt'):
            # (the reference's melting branch of the spectrum needs NumPy < 1.16's np.linspace: oracle/ref_shim.py)
            with ref_shim.numpy1_linspace():
                obs = get_radar_observables(subs, luts)
            d['numpy1_linspace'] = 1
        else:
            obs = get_radar_observables(subs, luts)
        for n in obs.values:
            d['obs_' + n] = np.asarray(obs.values[n])
        d['obs_mask'] = obs.mask
        d['n_valid'] = np.array([n_valid[h] for h in hl])
        # the sensitivity cut as get_PPI / get_RHI apply it: a list of LISTS of radials
        # (radar_operator.py:432-445), i.e. the branch that censors the Doppler spectrum bin by
        # bin (doppler_scatter.py:839-850); sensitivity of the case configuration
        import copy as _copy
        from cosmo_pol.scatter import cut_at_sensitivity
        cut = cut_at_sensitivity([[_copy.deepcopy(obs)]])[0][0]
        for n in cut.values:
            d['cutll_' + n] = np.asarray(cut.values[n])
        print(name, 'n_sub', len(subs), 'valid items', n_valid,
              'finite ZH', int(np.isfinite(obs.values['ZH']).sum()), '/', len(obs.values['ZH']))
        if name in BAD_VALUE_CASES:
            bad, counts = coverage_failures(name, d)
            print('  coverage', {k: counts[k] for k in COVERAGE[name]})
            assert not bad, (name, bad)
        out['radial_' + name] = d


def gen_lut_lookup(out):
    from cosmo_pol_amd import synthetic
    rng = np.random.default_rng(21)
    d = {}
    lr = ref_luts({'R': synthetic.make_lut('R', 5.6, '1mom', n_e=5),
                   'mS': synthetic.make_lut('mS', 5.6, '1mom', n_e=5)})
    e = rng.uniform(-1, 12, 200).astype(np.float32)
    e[:5] = [0, 2, 4, 1.9999999, 8]
    t = rng.uniform(255, 320, 200).astype(np.float32)
    t[:6] = [262, 264, 263.99997, 314, 316, 261.9]
    wc = rng.uniform(0, 1, 200)
    wc[:3] = [1e-3, 0.999, 0.5]
    # recover the bins the reference uses by looking up an index-coded table
    L = lr['R']
    code = np.zeros(L.value_table.shape[:2] + (1, 1))
    code[:, :, 0, 0] = np.arange(L.value_table.shape[0])[:, None] * 1000 + np.arange(L.value_table.shape[1])[None]
    vt = L.value_table
    L.value_table = code
    d['R_code'] = L.lookup_line(e=e, t=t)[:, 0, 0]
    L.value_table = vt
    L = lr['mS']
    code = np.zeros(L.value_table.shape[:2] + (1, 1))
    code[:, :, 0, 0] = np.arange(L.value_table.shape[0])[:, None] * 1000 + np.arange(L.value_table.shape[1])[None]
    vt = L.value_table
    L.value_table = code
    d['mS_code'] = L.lookup_line(e=e, wc=wc)[:, 0, 0]
    L.value_table = vt
    d.update(e=e, t=t, wc=wc)
    out['lut_lookup'] = d


def gen_aliasing(out):
    from cosmo_pol.utilities import aliasing
    rng = np.random.default_rng(3)
    v = rng.uniform(-40, 40, 200)
    v[:4] = [0.0, 8.3, -8.3, 16.6]
    d = dict(v=v)
    for i, nyq in enumerate([8.3, 12.4, 5.0]):
        d['nyq_%d' % i] = np.float64(nyq)
        d['folded_%d' % i] = aliasing(v.copy(), nyq)
    out['aliasing'] = d


def gen_lut_file(out):
    """A .lut file written by the product (cosmo_pol_amd.lut.save_lut) is read by the
    REFERENCE's load_lut and queried with the reference's lookup_line; the query
    results are the fixture (the file itself is regenerated by the test)."""
    import tempfile
    from cosmo_pol.lookup import lut as ref_lut
    from cosmo_pol_amd import lut as our_lut
    from cosmo_pol_amd import synthetic
    rng = np.random.default_rng(5)
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        for h in ['S', 'mG']:
            table = synthetic.make_lut(h, 9.41, '1mom', n_e=3, n_t=5)
            path = os.path.join(tmp, our_lut.lut_filename(h, 9.41, '1mom'))
            our_lut.save_lut(table, path)
            L = ref_lut.load_lut(path)
            if not isinstance(L.axes_names, dict):
                # NumPy >= 2: `ndarray.all()` of the 0-d object array no longer returns the
                # dict itself (lut.py:147-148); every other member is what the reference read
                L.axes_names = dict(table.axes_names)
            e = rng.uniform(0, 6, 20).astype(np.float32)
            ax = np.asarray(table.axes[1])
            t = rng.uniform(ax[0], ax[-1], 20).astype(np.float32)
            kw = {'e': e, ('wc' if h == 'mG' else 't'): t}
            got = L.lookup_line(**kw)
            assert got.shape == (20, 1024, 12)
            d[h + '_e'], d[h + '_t'] = e, t
            d[h + '_sum_d'] = got.sum(axis=1)          # [20, 12] is enough to pin the slices
            d[h + '_shape'] = np.array(L.value_table.shape)
    out['lut_file'] = d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(HERE), 'tests', 'golden'))
    ap.add_argument('--only', default=None)
    ap.add_argument('--cases', default=None, help='comma-separated radial case names (with --only radials)')
    args = ap.parse_args()
    ref_shim.load_reference()
    os.makedirs(args.out, exist_ok=True)
    out = {}
    gens = dict(gate_kernel=gen_gate_kernel, trajectory=gen_trajectory, quadrature=gen_quadrature,
                psd=gen_psd, pol=gen_pol, lut_lookup=gen_lut_lookup, radials=gen_radials,
                aliasing=gen_aliasing, lut_file=gen_lut_file)
    for k, g in gens.items():
        if args.only and k != args.only:
            continue
        if k == 'radials' and args.cases:
            g(out, args.cases.split(','))
        else:
            g(out)
    for name, d in out.items():
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **d)
        print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
