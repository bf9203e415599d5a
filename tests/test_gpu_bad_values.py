"""Bad values in the MODEL DATA on the GPU: NaN, the reference's -9999 sentinel, negative mass densities, temperatures off
the tables' axes -- planted in rings of grid columns around the radar (oracle/gen_golden.py::plant_bad_values), so that every
ray of a sweep and every sub-beam of a ray crosses them.

The reference reads the gate mask off the interpolated values of variable 0 (interpolation.py:398-411: `== -9999` -> +1,
NaN -> -1, every variable NaN at a masked gate); bad values in any other variable leave the mask at 0 and reach only the
consumers of that variable.  The single radials with a reference-made fixture are in tests/test_gpu_parity.py and
tests/test_gpu_seam.py (the `bad_*` cases); here: every launch form on a planted sweep, the per-radial seam, the scan API,
the Doppler spectrum, and a clean cube before / after a planted one in the same operator.

Tolerances are the project's (tests/test_gpu_parity.py): polarimetric variables at 1e-5 relative with the operand-scaled atol
of the three phase-like ones (and its ledger), RVEL at atol 2e-4 m/s, masks and NaN patterns exact."""
import copy

import numpy as np
import pytest

import _cases
from cosmo_pol_oracle import beam, scatter
from cosmo_pol_oracle import config as ocfg

pytestmark = pytest.mark.gpu

GG = _cases.gen_golden
RTOL = 1e-5
POL = ['ZH', 'ZV', 'ZDR', 'RHOHV', 'KDP', 'ATT_H', 'ATT_V', 'DELTA_HV', 'PHIDP']
KEYS = POL + ['RVEL', 'mask']
HYD_CUBE = ('R', 'S', 'G', 'I')

# every kind of planting within the 30 km (13.6 grid cells) of the sweep's rays; at 4 deg the rays cross the 0 C level
# ~8 cells out, so rain, the melting layer and snow all meet a planting
SWEEP_PLANTING = [('U', np.nan, 1.5, 2.5), ('QR_v', np.nan, 4.0, 4.6), ('QS_v', 'neg', 5.5, 6.3), ('T', 330.0, 6.4, 6.9),
                  ('T', 150.0, 7.0, 7.6), ('U', -9999.0, 8.5, 11.5), ('QG_v', np.nan, 9.0, 9.5), ('W', np.nan, 11.8, 12.4),
                  ('T', np.nan, 12.6, 13.0), ('RHO', np.nan, 13.0, 13.6)]
SWEEP_EL = 4.0
ENV_KNOBS = ('CPOL_RARE_DIRECT', 'CPOL_GATE1', 'CPOL_FUSE_CLASSIFY', 'CPOL_FUSE_GATE1', 'CPOL_GATE1_SPECIES', 'CPOL_GATE1_RAY',
             'CPOL_PSD_RARE', 'CPOL_ITAB')
# the launch forms tests/test_gpu_edges.py enumerates, by environment knob (read when the context is created)
FORMS = [('sorted', {'CPOL_RARE_DIRECT': '0', 'CPOL_GATE1': '0'}, 1),          # the general sequence with the counting sort
         ('direct', {'CPOL_GATE1': '0'}, 1),                                    # ... with the items listed directly
         ('default', {}, 1),
         ('default_3_lanes', {}, 3),
         ('direct_two_kernels', {'CPOL_GATE1': '0', 'CPOL_FUSE_CLASSIFY': '0'}, 1),     # k_interp_sweep + k_classify
         ('interp_gate1', {'CPOL_FUSE_GATE1': '1'}, 1),                         # k_interp_gate1
         ('gate1_one_thread', {'CPOL_GATE1_SPECIES': '0'}, 1),                  # k_gate1
         ('gate1_melting', {'CPOL_GATE1': '2'}, 1),                             # k_gate1<true>: melting species inside
         ('gate1_melting_interp', {'CPOL_GATE1': '2', 'CPOL_FUSE_GATE1': '1'}, 1),
         ('gate1_ray', {'CPOL_GATE1_RAY': '1'}, 1),                             # k_gate1_ray + k_scan_rays
         ('gate1_ray_ticket', {'CPOL_GATE1_RAY': '3'}, 1)]                      # ... the scans inside the gate kernel


def _planted_cube(planting=SWEEP_PLANTING):
    from cosmo_pol_amd import synthetic
    cube = synthetic.small_test_cube(hydrometeors=HYD_CUBE)
    cube['data'] = {k: v.copy() for k, v in cube['data'].items()}
    return GG.plant_bad_values(cube, planting)


def _oracle_cube(cube):
    return beam.ModelCube({n: cube['data'][n].copy() for n in _cases.ORDER}, cube['zlevels'], cube['proj_info'],
                          cube['resolution'], _cases.ORDER)


def _sweep_config(n_gh, melting):
    import bench
    conf = bench.bench_config(True, 'c3' if melting else 'c2')
    conf['integration'].update(nh_GH=n_gh, nv_GH=n_gh)
    return conf


def _luts(conf):
    oc = ocfg.make_config(conf)
    return oc, {h: _cases.synthetic_lut(h, oc['radar']['frequency'], oc['microphysics']['scheme'])
                for h in ocfg.hydrometeor_list(oc)}


def _operator(conf, luts, cube, lanes=1, output_variables='only_radar'):
    from cosmo_pol_amd import RadarOperator
    op = RadarOperator(config=copy.deepcopy(conf), luts=luts, output_variables=output_variables, lanes=lanes)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    return op


def _tol(k, sz, conf):
    from cosmo_pol_oracle import constants as OK
    wl = OK.Derived(conf).WAVELENGTH
    res_km = conf['radar']['radial_resolution'] / 1000.
    kdp = np.nan_to_num(1e-3 * (180.0 / np.pi) * wl * (np.abs(sz[:, 8]) + np.abs(sz[:, 10])))
    return {'KDP': RTOL * kdp, 'PHIDP': RTOL * (np.cumsum(2 * kdp) * res_km + np.pi), 'DELTA_HV': RTOL * np.pi}.get(k, 0.0)


def _against_oracle(values, mask, oobs, conf, tag):
    sz = np.nan_to_num(oobs.sz_total.astype(np.float64))
    for k in POL:
        # (the variable first: the ledger of operand-scaled tolerances is keyed by the first word of the name)
        _cases.assert_close_nan(values[k], oobs.values[k], rtol=RTOL, atol=_tol(k, sz, conf), name='%s %s' % (k, tag))
    _cases.assert_close_nan(values['RVEL'], oobs.values['RVEL'], rtol=RTOL, atol=2e-4, name='RVEL ' + tag)
    assert np.array_equal(mask, oobs.mask), tag + ' mask'


def _effects(ocube, clean_ocube, oconf, olut, azs, el):
    """Oracle radials of the planted and of the clean cube -> (per-ray observables, counts of what the rays met)."""
    out, n = [], dict(m1=0, p1=0, mask0_nan=0, rvel_only=0, finite=0, gates=0)
    for az in azs:
        o = scatter.radar_observables(beam.interpolate_radial(ocube, oconf, az, el), olut, oconf, return_sz=True)
        c = scatter.radar_observables(beam.interpolate_radial(clean_ocube, oconf, az, el), olut, oconf)
        zh, czh = o.values['ZH'], c.values['ZH']
        n['m1'] += int(((o.mask < 0) & (c.mask == 0)).sum())
        n['p1'] += int(((o.mask > 0) & (c.mask == 0)).sum())
        n['mask0_nan'] += int(((o.mask == 0) & np.isnan(zh) & np.isfinite(czh)).sum())
        n['rvel_only'] += int((np.isfinite(zh) & np.isnan(o.values['RVEL']) & np.isfinite(c.values['RVEL'])).sum())
        n['finite'] += int(np.isfinite(zh).sum())
        n['gates'] += zh.size
        out.append(o)
    return out, n


@pytest.mark.parametrize('melting', [False, True])
@pytest.mark.parametrize('n_gh', [1, 3])
def test_every_launch_form_gives_the_same_bits_on_a_planted_sweep(monkeypatch, n_gh, melting):
    """24 rays over the planted cube, one / nine sub-beams, without / with the melting species, through every launch form:
    all outputs and the counters equal those of the general sequence with the counting sort; with the integral tables off
    (CPOL_ITAB=0: every item integrated bin by bin, values equal to the tables' to ~1e-10 but not bit for bit) masks, NaN
    patterns and the item count are equal and its values meet the oracle on EVERY ray.  The counting sort and the default
    form: 8 rays against the oracle (the other forms carry the same bits)."""
    conf = _sweep_config(n_gh, melting)
    oconf, luts = _luts(conf)
    olut = {h: _cases.as_oracle_lut(l) for h, l in luts.items()}
    cube = _planted_cube()
    az = np.arange(0.0, 360.0, 15.0)
    el = np.full(len(az), SWEEP_EL)
    results = {}
    for mode, env, lanes in FORMS + [('no_integral_tables', {'CPOL_ITAB': '0'}, 1)]:
        for k in ENV_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        op = _operator(conf, luts, cube, lanes=lanes)
        res = op.simulate_rays(az, el, apply_sensitivity=False)
        c = op._ctx.counters()
        results[mode] = ({k: res[k].copy() for k in KEYS}, int(c.n_valid_items), int(c.n_subbeam_gates))
        op.close()
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    ref, n_items, n_sbg = results['sorted']
    assert n_items > 500 and n_sbg == len(az) * ref['ZH'].shape[1] * n_gh * n_gh
    for mode, (got, n_got, sbg_got) in results.items():
        assert (n_got, sbg_got) == (n_items, n_sbg), mode
        assert np.array_equal(got['mask'], ref['mask']), mode
        for k in KEYS:
            if mode == 'no_integral_tables':
                assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (mode, k)
            else:
                assert np.array_equal(got[k], ref[k], equal_nan=True), (mode, k)
    # ---- against the oracle; the rings make every ray cross every planting ----
    sample = list(range(0, len(az), 3))
    assert len(sample) >= 8
    oobs, n = _effects(_oracle_cube(cube), _oracle_cube(_planted_cube([])), oconf, olut, az, SWEEP_EL)
    print('planted sweep n_gh=%d melting=%s: %s' % (n_gh, melting, n))
    assert n['m1'] >= 5 * len(az) and n['p1'] >= 5 * len(az), n               # masks born from the data, on every ray
    assert n['mask0_nan'] >= 5 and n['rvel_only'] >= 5, n
    assert 3 * n['finite'] >= n['gates'], n
    for mode, rays in (('sorted', sample), ('default', sample), ('no_integral_tables', range(len(az)))):
        got = results[mode][0]
        for r in rays:
            _against_oracle({k: got[k][r] for k in KEYS}, got['mask'][r], oobs[r], oconf, '%s az=%g' % (mode, az[r]))


@pytest.mark.parametrize('n_gh', [1, 3])
def test_the_seam_carries_the_masks(n_gh):
    """interpolate_rays on the planted cube: mask and NaN pattern of the oracle's sub-beams; simulate_columns on them: the
    sweep's bits; get_interpolated_radial / integrate_radials: the oracle's records and antenna-averaged model variables.
    Then columns edited by the caller (NaN in QR_v, negative QS_v, mask left at 0) against the oracle on the same records."""
    from cosmo_pol_amd import radial
    conf = _sweep_config(n_gh, True)
    oconf, luts = _luts(conf)
    olut = {h: _cases.as_oracle_lut(l) for h, l in luts.items()}
    cube = _planted_cube()
    ocube, clean_ocube = _oracle_cube(cube), _oracle_cube(_planted_cube([]))
    op = _operator(conf, luts, cube, output_variables='all')
    az = np.array([20.0, 140.0, 260.0])
    el = np.full(3, SWEEP_EL)
    ref = op.simulate_rays(az, el, apply_sensitivity=False)
    cols = op.interpolate_rays(az, el, melting=True)
    n_born = 0
    for r in range(3):
        subs = beam.interpolate_radial(ocube, oconf, az[r], el[r])
        clean = beam.interpolate_radial(clean_ocube, oconf, az[r], el[r])
        assert cols['mask'].shape[1] == len(subs)
        for s, sb in enumerate(subs):
            assert np.array_equal(cols['mask'][r, s].astype(float), sb.mask), (r, s)
            for k, v in sb.values.items():
                assert np.array_equal(cols[k][r, s], v, equal_nan=True), (r, s, k)
            n_born += int(((sb.mask != 0) & (clean[s].mask == 0)).sum())      # born from the data, not from the geometry
    assert n_born >= 3 * 10 * n_gh * n_gh, 'the data-born masks were not exercised'
    got = op.simulate_columns(cols)
    for k, v in ref.items():
        if k != 'n_sub':
            assert np.array_equal(got[k], v, equal_nan=True), k
    # ---- the per-radial records ----
    rads = op.get_interpolated_radial(az[1], el[1])
    subs = beam.interpolate_radial(ocube, oconf, az[1], el[1])
    for s, (rd, sb) in enumerate(zip(rads, subs)):
        assert np.array_equal(rd.mask, sb.mask), s
        for k, v in sb.values.items():
            assert np.array_equal(rd.values[k], v, equal_nan=True), (s, k)
    integ, ointeg = radial.integrate_radials(rads), beam.integrate_subbeams(copy.deepcopy(subs))
    for k, v in ointeg.values.items():
        _cases.assert_close_nan(integ.values[k], v, rtol=1e-12, name='integ:' + k)
    assert np.array_equal(integ.mask, ointeg.mask)
    names = op._staged_vars
    for i, nm in enumerate(names):
        _cases.assert_close_nan(ref['model_vars'][i][1], ointeg.values[nm], rtol=1e-12, name='model:' + nm)
    obs = op.get_radar_observables(rads)
    oobs = scatter.radar_observables(copy.deepcopy(subs), olut, oconf, return_sz=True)
    _against_oracle(obs.values, obs.mask, oobs, oconf, 'records:')
    for k in POL + ['RVEL']:
        assert np.array_equal(obs.values[k], ref[k][1], equal_nan=True), k
    # ---- edited by the caller: bad values under mask 0 (the melting fields of the records are kept as they are) ----
    # Each edit goes to gates where the species it touches holds an item, so that it changes the radial.
    rng = np.random.default_rng(5)
    before = oobs
    for sb in subs:
        v, inside = sb.values, np.asarray(sb.mask) == 0
        with np.errstate(invalid='ignore'):
            rain = np.where(inside & ((v['QR_v'] > 0) | (v['QmS_v'] > 0)))[0]
            snow = np.where(inside & (v['QS_v'] > 0))[0]
        assert len(rain) >= 8 and len(snow) >= 8, (len(rain), len(snow))
        gr, gs = rng.choice(rain, size=8, replace=False), rng.choice(snow, size=8, replace=False)
        v['QR_v'][gr[:4]] = np.nan
        v['T'][gr[4:6]] = np.float32(150.0)
        v['T'][gr[6:8]] = np.nan
        v['QS_v'][gs[:4]] = -v['QS_v'][gs[:4]]
        v['T'][gs[4:6]] = np.float32(330.0)
        v['T'][gs[6:8]] = np.float32(150.0)
    obs = op.get_radar_observables(subs)
    oobs = scatter.radar_observables(copy.deepcopy(subs), olut, oconf, return_sz=True)
    assert np.array_equal(oobs.mask, before.mask)                 # the masks were left as they were
    changed = ~np.isclose(oobs.values['ZH'], before.values['ZH'], rtol=1e-4, atol=0, equal_nan=True)
    assert changed.sum() >= 8, 'the edits changed ZH at %d gates only' % changed.sum()
    _against_oracle(obs.values, obs.mask, oobs, oconf, 'edited:')
    op.close()


def test_scan_api_masks_what_the_rays_mask():
    """get_PPI on the planted cube: every field is masked exactly where the per-ray result (sensitivity cut included) is
    NaN; the pipelined form (a sweep per lane) and the one-sequence form agree."""
    conf = _sweep_config(1, False)
    conf['radar']['sensitivity'] = [25., 10000]
    oconf, luts = _luts(conf)
    cube = _planted_cube()
    clean_ocube = _oracle_cube(_planted_cube([]))
    op = _operator(conf, luts, cube, lanes=3)
    azs = np.arange(0.0, 360.0, 30.0)
    elevs = [2.0, SWEEP_EL, 7.0]
    scan = op.get_PPI(elevs, azimuths=azs)
    op.pipeline_single_beam_scans = False
    one_seq = op.get_PPI(elevs, azimuths=azs)
    n_cut = n_nan = 0
    for i, e in enumerate(elevs):
        rays = op.simulate_rays(azs, np.full(len(azs), e), apply_sensitivity=True)
        raw = op.simulate_rays(azs, np.full(len(azs), e), apply_sensitivity=False)
        n_cut += int(np.isfinite(raw['ZH']).sum() - np.isfinite(rays['ZH']).sum())
        for name in POL + ['RVEL']:
            a = np.ma.asarray(scan.get_field(i, name))
            nan = np.isnan(rays[name])
            if name in ('ZH', 'ZV', 'ZDR'):                     # dB fields: 0 -> NaN (pyart_wrapper.py:256-258)
                nan = nan | (rays[name] == 0)
            assert np.array_equal(np.ma.getmaskarray(a), nan), (e, name)
            assert np.array_equal(np.asarray(scan.raw[i]['fields'][name]), rays[name], equal_nan=True), (e, name)
            b = np.ma.asarray(one_seq.get_field(i, name))
            assert np.array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b)), (e, name)
            assert np.array_equal(a.filled(0), b.filled(0)), (e, name)
        assert np.array_equal(scan.raw[i]['mask'], raw['mask'])
        # masks born from the data: the oracle's mask on the unplanted cube is 0 there
        clean_mask = np.array([beam.interpolate_radial(clean_ocube, oconf, a, e)[0].mask for a in azs])
        n_nan += int(((raw['mask'] != 0) & (clean_mask == 0)).sum())
    assert n_cut > 0, 'the sensitivity cut was not exercised'
    assert n_nan >= 10 * len(azs) * len(elevs), 'the data-born masks were not exercised'
    op.close()


def test_planted_spectrum_case_against_its_fixture(golden):
    """bad_d3_ice_sub through simulate_rays: the comparison of tests/test_gpu_broadening.py (exact NaN pattern, DSPECTRUM at
    rtol 2e-5 with the spectrum's operand-scaled atol and its ledger, RVEL at atol 2e-4 m/s)."""
    name = 'bad_d3_ice_sub'
    g = golden('radial_' + name)
    conf, az, el, ocube, luts, cube = _cases.radial_case(name)
    over = GG.radial_case_inputs(name)[0]
    op = _operator(over, luts, cube, output_variables='all')
    res = op.simulate_rays([az], [el], apply_sensitivity=False)
    sp, want = res['DSPECTRUM'][0], g['obs_DSPECTRUM']
    assert sp.shape == want.shape
    ok = ~np.isnan(want) & (want != 0)
    print('%s: DSPECTRUM worst pure relative deviation %.3e' % (name, np.max(np.abs(sp[ok] - want[ok]) / np.abs(want[ok]))))
    assert np.array_equal(np.isnan(sp), np.isnan(want))
    assert np.array_equal(sp == 0, want == 0)                   # the rows a planting emptied, and no others
    assert np.array_equal(np.isnan(res['RVEL'][0]), np.isnan(g['obs_RVEL']))
    _cases.assert_close_nan(sp, want, rtol=2e-5, atol=1e-6 * np.nanmax(want), name='golden:DSPECTRUM')
    _cases.assert_close_nan(res['RVEL'][0], g['obs_RVEL'], rtol=RTOL, atol=2e-4, name='golden:RVEL')
    for k in ['ZH', 'ZDR', 'RHOHV']:
        _cases.assert_close_nan(res[k][0], g['obs_' + k], rtol=RTOL, name='golden:' + k)
    assert np.array_equal(res['mask'][0], g['obs_mask'])
    cut = op.simulate_rays([az], [el], apply_sensitivity=True)
    for k in POL + ['RVEL', 'DSPECTRUM']:
        gk = g['cutll_' + k]
        assert np.array_equal(np.isnan(cut[k][0]), np.isnan(gk)), 'cut pattern: ' + k
        assert np.array_equal(cut[k][0][~np.isnan(gk)], res[k][0][~np.isnan(gk)]), k
    # the seam on the planted spectrum case
    got = op.simulate_columns(op.interpolate_rays([az], [el], melting=True))
    for k, v in res.items():
        if k != 'n_sub':
            assert np.array_equal(got[k], v, equal_nan=True), k
    op.close()


@pytest.mark.parametrize('name', ['c3_melt_ice', 'c4_subbeams'])
def test_clean_cube_before_and_after_a_planted_one(name):
    """One operator: the clean case, the planted cube of its bad-value twin, the clean case again -- identical bits before
    and after (no state of a data-dependent switch survives a staging), and the planted run equals a fresh operator's."""
    twin = {'c3_melt_ice': 'bad_c3_masks', 'c4_subbeams': 'bad_c4_sub15'}[name]
    conf, az, el, _, luts, cube = _cases.radial_case(name)
    planted = _cases.radial_case(twin)[5]
    over = GG.radial_case_inputs(name)[0]
    op = _operator(over, luts, cube, output_variables='all')
    before = op.simulate_rays([az], [el], apply_sensitivity=False)
    op.load_model_arrays(planted['data'], planted['zlevels'], planted['proj_info'], planted['resolution'])
    mid = op.simulate_rays([az], [el], apply_sensitivity=False)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    after = op.simulate_rays([az], [el], apply_sensitivity=False)
    op.close()
    fresh_op = _operator(over, luts, planted, output_variables='all')
    fresh = fresh_op.simulate_rays([az], [el], apply_sensitivity=False)
    fresh_op.close()
    assert not np.array_equal(mid['mask'], before['mask'])
    for k, v in before.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(after[k], v, equal_nan=True), k
            assert np.array_equal(mid[k], fresh[k], equal_nan=True), k
