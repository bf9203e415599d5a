"""Doppler-spectrum broadening by turbulence and antenna motion on the GPU (k_spec_width, k_spec_broaden): the filter on
explicit rows against the reference's broaden_spectrum (tests/golden/broaden_rows.npz), and every broadening fixture through
simulate_rays and through the per-radial seam.  The fixtures are the reference's own output (tools/gen_golden_broadening.py,
one emulation: the module-level CONFIG of doppler_scatter.py rebound to the live configuration).

Tolerances are the project's: DSPECTRUM at rtol 2e-5 with the spectrum's operand-scaled atol (counted by the ledger of
_cases.assert_close_nan), RVEL at atol 2e-4 m/s.  The NaN pattern and the sub-beam switch are compared exactly.  The worst pure
relative deviation of every fixture is printed and, when CPOL_PARITY_DIR names a directory, appended to
broadening_parity_records.jsonl there (profiles/ keeps a copy)."""
import copy
import json
import os

import numpy as np
import pytest

import _broadening as B
import _cases
from cosmo_pol_oracle import config as ocfg

pytestmark = pytest.mark.gpu

RTOL = 1e-5
OUT = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL', 'DSPECTRUM']


def _record(**kw):
    out = os.environ.get('CPOL_PARITY_DIR')
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'broadening_parity_records.jsonl'), 'a') as f:
        f.write(json.dumps(kw) + '\n')


def _worst_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = ~np.isnan(b) & (b != 0)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0


def _operator(over, cube, with_model=True):
    from cosmo_pol_amd import RadarOperator
    conf = ocfg.make_config(over)
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme'])
            for h in ocfg.hydrometeor_list(conf)}
    op = RadarOperator(config=copy.deepcopy(over), luts=luts)
    if with_model:
        op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    return op


def _setup(name, **kw):
    over, az, el, cube, two = B.case_inputs(name)
    return _operator(over, cube, **kw), az, el, cube


def _stored_subradials(g):
    """The reference's sub-radials of a fixture as records get_radar_observables takes."""
    from cosmo_pol_amd.radial import Radial
    geometry = ('mask', 'lats', 'lons', 's', 'h', 'e', 'has_melting', 'spec_raw', 'spec_broad', 'width', 'switch', 'ah')
    subs = []
    for s in range(int(g['n_sub'])):
        pre = 'sub%d_' % s
        values = {k[len(pre):]: g[k].copy() for k in g.files if k.startswith(pre) and k[len(pre):] not in geometry}
        r = Radial(values, g[pre + 'mask'].copy(), g[pre + 'lats'], g[pre + 'lons'], g[pre + 's'], g[pre + 'h'],
                   elev_profile=g[pre + 'e'].copy(), quad_pt=[float(x) for x in g['quad_pts'][s]], quad_weight=float(g['quad_w'][s]))
        r.has_melting = bool(g[pre + 'has_melting'])
        subs.append(r)
    return subs


def test_broaden_rows_against_reference(golden):
    """cpol_broaden_rows == the reference's broaden_spectrum on the rows of broaden_rows.npz: radius 0 to radius >> n_v, a
    one-bin row, an all-zero row (NaN)."""
    from cosmo_pol_amd import _native as N
    g = golden('broaden_rows')
    ctx = N.Context(0)
    for n_v in (33, 65, 257):
        rows, sig, want = g['rows_%d' % n_v], g['sigma_%d' % n_v], g['out_%d' % n_v]
        got = ctx.broaden_rows(rows, sig)
        assert got.dtype == np.float32 and got.shape == want.shape
        worst = _worst_rel(got, want)
        print('broaden_rows n_v=%d worst pure relative deviation %.3e, bit-equal rows %d / %d'
              % (n_v, worst, int((got.view(np.uint32) == want.view(np.uint32)).all(1).sum()), len(sig)))
        _record(fixture='broaden_rows', n_v=n_v, worst_pure_rel=worst)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        _cases.assert_close_nan(got, want, rtol=2e-5, name='broaden_rows:%d' % n_v)
        assert np.array_equal((got > 0), (want > 0))              # the support: radius and reflection
    ctx.close()


def test_broaden_rows_chosen_rows():
    """Rows chosen for the filter, against the NumPy restatement (scipy.ndimage.gaussian_filter on the host): NaN in a row,
    sigma 0 and NaN (identity), long rows on the 256-thread form (n_v = 1025, 4097) with radii below and beyond n_v."""
    from cosmo_pol_amd import _native as N
    ctx = N.Context(0)
    rng = np.random.default_rng(11)
    for n_v, sig in ((33, [0.0, np.nan, 1e-16, 2.0, 2.0, 40.0]), (1024, [0.3, 5.0, 300.0, 5000.0, 0.0, 7.5]),
                     (1025, [0.3, 5.0, 300.0, 5000.0, 0.0, 7.5]), (4097, [0.7, 3.0, 90.0, 1100.0, 20000.0, 12.0])):
        rows = (rng.random((len(sig), n_v)) ** 6).astype(np.float32)
        rows[rows < 0.2] = 0
        rows[4, n_v // 2] = np.nan                             # a NaN in the row reaches every bin through the rescale
        sig = np.array(sig, dtype=np.float64)
        got = ctx.broaden_rows(rows, sig)
        host_sig = np.where(np.isnan(sig), 0.0, sig)           # (gaussian_filter's own guard: sigma not above 1e-15 = identity)
        want = B.broaden_rows(rows, host_sig)
        print('chosen rows n_v=%d worst pure relative deviation %.3e' % (n_v, _worst_rel(got, want)))
        assert np.isnan(got[4]).all() and np.isnan(want[4]).all()
        _cases.assert_close_nan(got, want, rtol=2e-5, name='chosen:%d' % n_v)
        if n_v == 33:
            for i in (0, 1, 2):                                # identity, then the rescale
                assert np.array_equal(got[i], rows[i] / rows[i].sum() * rows[i].sum())
    with pytest.raises(ValueError):
        ctx.broaden_rows(np.zeros((2, 1), np.float32), np.ones(2))
    with pytest.raises(ValueError):
        ctx.broaden_rows(np.zeros((1, 5000), np.float32), np.ones(1))
    assert np.isfinite(ctx.broaden_rows(np.ones((1, 8), np.float32), np.ones(1))).all()      # usable after a refusal
    ctx.close()


@pytest.mark.parametrize('name', list(B.CASES))
def test_fixture_through_sweep_and_seam(golden, name):
    g = golden('radial_' + name)
    op, az, el, cube = _setup(name)
    conf = op.config
    turb = bool(conf['doppler']['turbulence_correction'])
    assert ('EDR' in op._staged_vars) == turb
    res = op.simulate_rays([az], [el], apply_sensitivity=False)
    sp, want = res['DSPECTRUM'][0], g['obs_DSPECTRUM']
    assert sp.shape == want.shape
    worst_sp, worst_rv = _worst_rel(sp, want), float(np.nanmax(np.abs(res['RVEL'][0] - g['obs_RVEL'])))
    print('%s: DSPECTRUM worst pure relative deviation %.3e, RVEL worst absolute deviation %.3e m/s, NaN gates %d / %d'
          % (name, worst_sp, worst_rv, int(np.isnan(want).all(1).sum()), want.shape[0]))
    _record(fixture='radial_' + name, worst_pure_rel_DSPECTRUM=worst_sp, worst_abs_RVEL=worst_rv,
            bit_equal_bins=int((sp == want).sum()), bins=int((~np.isnan(want)).sum()))
    # ---- the reference's spectrum, RVEL and NaN pattern (every gate and bin; a NaN is compared as a NaN) ----
    assert np.array_equal(np.isnan(sp), np.isnan(want))
    assert np.array_equal(np.isnan(res['RVEL'][0]), np.isnan(g['obs_RVEL']))
    _cases.assert_close_nan(sp, want, rtol=2e-5, atol=1e-6 * np.nanmax(want), name='golden:DSPECTRUM')
    _cases.assert_close_nan(res['RVEL'][0], g['obs_RVEL'], rtol=RTOL, atol=2e-4, name='golden:RVEL')
    for k in ['ZH', 'ZDR', 'RHOHV']:
        _cases.assert_close_nan(res[k][0], g['obs_' + k], rtol=RTOL, name='golden:' + k)
    assert np.array_equal(res['mask'][0], g['obs_mask'])
    # ---- the bin-wise sensitivity cut ----
    cut = op.simulate_rays([az], [el], apply_sensitivity=True)
    for k in OUT:
        gk = g['cutll_' + k]
        assert np.array_equal(np.isnan(cut[k][0]), np.isnan(gk)), 'cut pattern: ' + k
        assert np.array_equal(cut[k][0][~np.isnan(gk)], res[k][0][~np.isnan(gk)]), k
    # ---- the seam: the reference's stored sub-radials, and the library's own export ----
    subs = _stored_subradials(g)
    obs = op.get_radar_observables(subs)
    for k in OUT:
        same = np.array_equal(obs.values[k], res[k][0], equal_nan=True)
        if not same:
            print('%s: get_radar_observables(stored sub-radials) differs from simulate_rays in %s, worst relative %.3e'
                  % (name, k, _worst_rel(obs.values[k], res[k][0])))
        assert same, k
    cols = op.interpolate_rays([az], [el], melting=True)
    assert ('EDR' in cols) == turb
    for s in range(int(g['n_sub'])):
        if turb:
            assert np.array_equal(cols['EDR'][0, s], g['sub%d_EDR' % s], equal_nan=True), s
    got = op.simulate_columns(cols)
    assert set(got) == set(res)
    for k, v in res.items():
        if k != 'n_sub':
            assert np.array_equal(got[k], v, equal_nan=True), k
    if turb:
        with pytest.raises(ValueError):
            op.simulate_columns({k: v for k, v in cols.items() if k != 'EDR'})
    rads = op.get_interpolated_radial(az, el)
    assert all(('EDR' in r.values) == turb for r in rads)
    obs2 = op.get_radar_observables(rads)
    for k in OUT:
        assert np.array_equal(obs2.values[k], res[k][0], equal_nan=True), k
    op.close()


def test_switches_off_are_bit_identical_and_meet_the_unbroadened_golden(golden, capsys):
    """A context that broadened a sweep, then runs with both switches off == a context that never saw the feature; a model
    with EDR but no switch stages nothing more; turbulence without EDR in the model prints the reference's notice and equals
    the switch being off."""
    base = 'd3_1mom_ice_sub'
    g = golden('radial_' + base)
    over0, az, el, cube0, _ = _cases.gen_golden.radial_case_inputs(base)
    fresh = _operator(over0, cube0)
    want = fresh.simulate_rays([az], [el], apply_sensitivity=False)
    n_model = want['model_vars'].shape[0]
    fresh.close()
    atol = 1e-6 * np.nanmax(g['obs_DSPECTRUM'])
    _cases.assert_close_nan(want['DSPECTRUM'][0], g['obs_DSPECTRUM'], rtol=2e-5, atol=atol, name='golden:DSPECTRUM')
    _cases.assert_close_nan(want['RVEL'][0], g['obs_RVEL'], rtol=RTOL, atol=2e-4, name='golden:RVEL')

    op, az, el, cube = _setup('d3_turb_motion_sub')
    on = op.simulate_rays([az], [el], apply_sensitivity=False)
    assert on['model_vars'].shape[0] == n_model + 1 and op._staged_vars[-1] == 'EDR'
    assert not np.array_equal(on['DSPECTRUM'], want['DSPECTRUM'], equal_nan=True)
    conf = op.config
    conf['doppler']['turbulence_correction'] = conf['doppler']['motion_correction'] = 0
    op.config = conf
    off = op.simulate_rays([az], [el], apply_sensitivity=False)
    assert 'EDR' not in op._staged_vars
    assert set(off) == set(want)
    for k, v in want.items():
        if k != 'n_sub':
            assert off[k].shape == v.shape and np.array_equal(off[k], v, equal_nan=True), k
    # back on: the cube is staged with EDR again and the first result returns
    conf['doppler']['turbulence_correction'] = conf['doppler']['motion_correction'] = 1
    op.config = conf
    again = op.simulate_rays([az], [el], apply_sensitivity=False)
    for k in OUT + ['model_vars']:
        assert np.array_equal(again[k], on[k], equal_nan=True), k
    op.close()

    # turbulence asked for, no EDR in the model
    over = copy.deepcopy(over0)
    over['doppler']['turbulence_correction'] = 1
    capsys.readouterr()
    op = _operator(over, cube0)
    assert 'No  turbulence correction will be done' in capsys.readouterr().out
    assert op.config['doppler']['turbulence_correction'] == 0 and 'EDR' not in op._staged_vars
    res = op.simulate_rays([az], [el], apply_sensitivity=False)
    for k, v in want.items():
        if k != 'n_sub':
            assert np.array_equal(res[k], v, equal_nan=True), k
    op.close()


def test_refused_calls_leave_the_context_usable(monkeypatch):
    """CPOL_ERR_ARG: turbulence without a staged EDR index, broadening outside Doppler scheme 3, no bin width."""
    from cosmo_pol_amd import _native as N
    op, az, el, cube = _setup('d3_turb_motion_sub')
    good = op.simulate_rays([az], [el], apply_sensitivity=False)
    real = N.Context.run_sweep
    for edit in (lambda p: setattr(p, 'var_edr', -1), lambda p: setattr(p, 'var_edr', 99),
                 lambda p: setattr(p, 'simulate_doppler', 1), lambda p: setattr(p, 'v_res', 0.0)):
        def bad(self, params, tables, outputs, edit=edit):
            q = N.SweepParams.from_buffer_copy(params)
            edit(q)
            return real(self, q, tables, outputs)
        monkeypatch.setattr(N.Context, 'run_sweep', bad)
        with pytest.raises(ValueError):
            op.simulate_rays([az], [el], apply_sensitivity=False)
        monkeypatch.setattr(N.Context, 'run_sweep', real)
        again = op.simulate_rays([az], [el], apply_sensitivity=False)
        for k in OUT:
            assert np.array_equal(again[k], good[k], equal_nan=True), k
    op.close()


def test_scans_run_with_both_switches():
    """get_PPI / get_RHI / get_VPROF go through the same launch sequence: rows of a PPI equal simulate_rays."""
    op, az, el, cube = _setup('d3_turb_motion_sub')
    azs = [az, az + 1.0]
    want = op.simulate_rays(azs, [el, el], apply_sensitivity=True)
    scan = op.get_PPI(elevations=[el], azimuths=azs)
    assert scan is not None
    assert np.array_equal(np.asarray(scan.raw[0]['fields']['RVEL']), want['RVEL'], equal_nan=True)
    assert op.get_RHI(azimuths=[az], elevations=[el, el + 1.0]) is not None
    assert op.get_VPROF() is not None
    op.close()
