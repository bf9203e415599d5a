"""Doppler-spectrum broadening (turbulence and antenna motion): the shared inputs of the `radial_d3_*` broadening fixtures
and a NumPy restatement of what the reference does between get_doppler_spectrum and the attenuation correction
(scatter/doppler_scatter.py:360-369, 727-801).  tools/gen_golden_broadening.py and the tests import this module; the
product never does (its filter runs on the device)."""
import numpy as np

import gen_golden  # oracle/gen_golden.py

A_TURB = 1.6       # global_constants.py:124

# name -> (base case of oracle/gen_golden.py, configuration overrides, elevation override or None)
CASES = {
    'd3_turb_motion_sub': ('d3_1mom_ice_sub', {'doppler': {'turbulence_correction': 1, 'motion_correction': 1}}, None),
    'd3_turb_fft256': ('d3_1mom_ice_sub', {'radar': {'FFT_length': 256}, 'integration': {'nh_GH': 1, 'nv_GH': 1},
                                           'doppler': {'turbulence_correction': 1}}, None),
    'd3_turb_motion_fft256': ('d3_1mom_ice_sub', {'radar': {'FFT_length': 256}, 'integration': {'nh_GH': 1, 'nv_GH': 1},
                                                  'doppler': {'turbulence_correction': 1, 'motion_correction': 1}}, None),
    'd3_motion_melt': ('d3_melt', {'doppler': {'motion_correction': 1}}, None),
    # three vertical nodes; the range ends where only the uppermost sub-beam has left the top of the cube
    # (119 gates of 300 m at 35 deg: the sub-beams leave the top at gates 120 / 119 / 117)
    'd3_turb_masked': ('d3_1mom_ice_sub', {'radar': {'range': 35700}, 'integration': {'nh_GH': 1, 'nv_GH': 3},
                                           'doppler': {'turbulence_correction': 1}}, None),
    # bad values in the model data under the turbulence switch (see PLANTINGS below): the base case is d3_turb_motion_sub
    'bad_d3_turb_edr': ('d3_1mom_ice_sub', {'doppler': {'turbulence_correction': 1, 'motion_correction': 1}}, None),
    'bad_d3_turb_umask': ('d3_1mom_ice_sub', {'doppler': {'turbulence_correction': 1, 'motion_correction': 1}}, None),
}

# rings of grid columns (oracle/gen_golden.py::plant_bad_values) planted into the cube AFTER the EDR field was added.
# NaN in EDR leaves the mask at 0 and makes the turbulence width of those gates NaN; NaN in U masks the gates (-1, from the
# data) and with them EDR.  Either way `np.sum(width) > 0` is false and the sub-beam stays unbroadened (quirk Q13) -- every
# sub-beam, since a ring is crossed by all of them -- while d3_turb_motion_sub, the same configuration on the clean cube, is
# broadened in all three.
PLANTINGS = {
    'bad_d3_turb_edr': [('EDR', np.nan, 2.4, 3.0)],
    'bad_d3_turb_umask': [('U', np.nan, 6.0, 7.5)],
}
CLEAN_TWIN = {'bad_d3_turb_edr': 'd3_turb_motion_sub', 'bad_d3_turb_umask': 'd3_turb_motion_sub'}
MIN_EFFECT_GATES = 5


def coverage_failures(name, g, clean):
    """What a planted broadening fixture `g` must show, against the fixture `clean` of its twin on the unplanted cube; ->
    (list of unmet conditions, counts).  Checked by the generator and asserted again by tests/test_bad_value_fixtures.py."""
    n_sub = int(g['n_sub'])
    c = {'switch': [int(g['sub%d_switch' % s]) for s in range(n_sub)],
         'clean_switch': [int(clean['sub%d_switch' % s]) for s in range(n_sub)]}
    nan_edr_mask0, born = [], []
    for s in range(n_sub):
        m, mc = g['sub%d_mask' % s], clean['sub%d_mask' % s]
        nan_edr_mask0.append(int(((m == 0) & np.isnan(g['sub%d_EDR' % s]) & np.isnan(g['sub%d_width' % s])).sum()))
        born.append(int(((m == -1) & (mc == 0) & np.isnan(g['sub%d_EDR' % s])).sum()))
    sp = g['obs_DSPECTRUM']
    row = np.isfinite(sp).all(axis=1) & (sp != 0).any(axis=1)
    c.update(nan_edr_mask0=nan_edr_mask0, mask_m1_data=born, rows_kept=int(row.sum()),
             bins_kept=int((np.isfinite(sp) & (sp != 0)).sum()), finite_ZH=int(np.isfinite(g['obs_ZH']).sum()),
             n_gates=int(g['obs_ZH'].size), differs_from_clean=not np.array_equal(sp, clean['obs_DSPECTRUM'], equal_nan=True))
    want = nan_edr_mask0 if name == 'bad_d3_turb_edr' else born
    bad = []
    if min(want) < MIN_EFFECT_GATES:
        bad.append('planting met at %s gates of the sub-beams' % want)
    if name == 'bad_d3_turb_edr' and any(born):
        bad.append('NaN EDR must leave the masks alone: %s' % born)
    if any(c['switch']) or not all(c['clean_switch']):
        bad.append('switch %s, on the clean cube %s' % (c['switch'], c['clean_switch']))
    if c['rows_kept'] < 20 or c['bins_kept'] < 40 or 3 * c['finite_ZH'] < c['n_gates'] or not c['differs_from_clean']:
        bad.append('too little left: %s' % c)
    return bad, c


def edr_field(shape, seed=20261016):
    """The eddy dissipation rate of the fixtures: positive and varying, 1e-4 + 5e-3 U(0, 1) in float32, a seeded function of
    the cube shape."""
    rng = np.random.default_rng([seed] + [int(n) for n in shape])
    return (1e-4 + 5e-3 * rng.random(tuple(shape))).astype(np.float32)


def case_inputs(name):
    """-> (configuration overrides, azimuth, elevation, cube with EDR when the case needs it, two-moment flag)"""
    base, extra, el_over = CASES[name]
    over, az, el, cube, two = gen_golden.radial_case_inputs(base)
    for sec, dd in extra.items():
        over.setdefault(sec, {}).update(dd)
    if over['doppler'].get('turbulence_correction'):
        cube['data']['EDR'] = edr_field(cube['data']['T'].shape)
    if name in PLANTINGS:
        gen_golden.plant_bad_values(cube, PLANTINGS[name])
    return over, az, (el if el_over is None else el_over), cube, two


def width_turb(ranges, edr, radial_resolution, beamwidth_deg):
    """spectral_width_turb (:727-758) under NumPy-2 promotion: float32 `edr` times Python floats stays float32."""
    sigma_r = 0.35 * radial_resolution
    sigma_theta = np.deg2rad(beamwidth_deg) / (4. * np.sqrt(np.log(2)))
    out = np.zeros((len(edr),))
    with np.errstate(invalid='ignore'):
        near = sigma_r < 0.1 * ranges * sigma_theta
        out[near] = ((ranges[near] * edr[near] * sigma_theta * A_TURB ** (3 / 2.)) / 0.72) ** (1 / 3.)
        far = sigma_r >= 0.1 * ranges * sigma_theta
        out[far] = (((edr[far] * sigma_r * (1.35 * A_TURB) ** (3 / 2))
                     / (11. / 15. + 4. / 15. * (ranges[far] * sigma_theta / sigma_r) ** 2) ** (-3 / 2.)) ** (1 / 3.))
    return out


def width_motion(elev_folded, wavelength_mm, antenna_speed, beamwidth_deg):
    """spectral_width_motion (:760-777); `wavelength_mm / 100` is the reference's statement."""
    wavelength = wavelength_mm / 100.
    return (wavelength * antenna_speed * np.cos(np.deg2rad(elev_folded))) / (2 * np.pi * np.deg2rad(beamwidth_deg))


def fold(elev):
    e = np.array(elev, copy=True)
    e[e > 90] = 180 - e[e > 90]
    e[e < 0] = -e[e < 0]
    return e


def width(conf, wavelength_mm, ranges, edr, elev):
    """The width vector of one sub-beam (:361-366): the two standard deviations added linearly."""
    w = np.zeros(len(elev))
    if conf['doppler']['turbulence_correction']:
        w += width_turb(ranges, edr, conf['radar']['radial_resolution'], conf['radar']['3dB_beamwidth'])
    if conf['doppler']['motion_correction']:
        w += width_motion(fold(elev), wavelength_mm, conf['radar']['antenna_speed'], conf['radar']['3dB_beamwidth'])
    return w


def switch(w):
    """:368 -- a NaN anywhere makes the sum NaN and the comparison false."""
    with np.errstate(invalid='ignore'):
        return bool(np.sum(w) > 0)


def broaden_rows(rows, sigma_bins):
    """broaden_spectrum (:779-801) on float32 rows with sigma in bins: gaussian_filter per row, then the rescale to the
    original float32 row sum (an empty row becomes NaN)."""
    from scipy.ndimage import gaussian_filter
    spec = np.array(rows, dtype=np.float32, copy=True)
    orig = np.sum(spec, 1)
    for i, s in enumerate(sigma_bins):
        spec[i, :] = gaussian_filter(spec[i, :], s)
    conv = np.sum(spec, 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return spec / conv[:, None] * orig[:, None]


def broaden(spec, w, varray):
    v_res = varray[2] - varray[1]
    return broaden_rows(spec, [t / v_res for t in w])


def function_rows(seed=5):
    """The rows of tests/golden/broaden_rows.npz: per n_v seeded float32 rows with sigma from 0.05 bins (radius 0) to 3 n_v,
    a one-bin row and an all-zero row.  -> list of (rows [n, n_v] float32, sigma_bins [n] float64)"""
    out = []
    for n_v in (33, 65, 257):
        rng = np.random.default_rng([seed, n_v])
        sig = np.array([0.05, 0.12, 0.3, 0.8, 1.4, 3.7, 11.0, 0.4 * n_v, 1.0 * n_v, 3.0 * n_v, 2.5, 2.5, 0.05, 6.1])
        rows = (rng.random((len(sig), n_v)) ** 4 * 10 ** rng.uniform(-3, 3, (len(sig), 1))).astype(np.float32)
        rows[rows < np.float32(0.05) * rows.max(1, keepdims=True)] = 0          # sparse spectra, as the reference's
        rows[10] = 0
        rows[10, n_v // 3] = np.float32(7.25)                                   # a single occupied bin
        rows[11] = 0                                                            # no power: 0 / 0
        rows[12] = 0
        rows[12, 0] = np.float32(1.5)                                           # one bin at the edge, radius 0
        rows[13, :3] = np.float32(2.0)                                          # power at the reflecting boundary
        out.append((rows, sig))
    return out
