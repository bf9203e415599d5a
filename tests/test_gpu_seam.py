"""The per-radial seam on the GPU: cpol_interp_subbeams (interpolate_rays, get_interpolated_radial) against the oracle's
interpolate_radial, and cpol_run_columns (simulate_columns, get_radar_observables) on sub-radials the caller hands in --
the oracle's, edited ones, device-resident torch columns, the library's own export -- against cpol_run_sweep's bits and
the oracle."""
import copy

import numpy as np
import pytest

import _cases
from cosmo_pol_oracle import beam, scatter

pytestmark = pytest.mark.gpu

RTOL = 1e-5
OUT = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL', 'DSPECTRUM']
# the launch forms a column call shares with the sweep (the interpolating ones, k_interp_classify / k_interp_gate1, excluded)
SHARED_FORMS = ('g1r', 'gate1_ray', 'gate1', 'rare_direct', 'subbeam_sum', 'final_inplace', 'n_sub')


def _assert_forms(op, sweep_forms):
    forms = op._ctx.launch_forms()
    assert forms['interp_classify'] == 0 and forms['graph_replayed'] == 0
    for k in SHARED_FORMS:
        assert forms[k] == sweep_forms[k], (k, forms, sweep_forms)
    return forms


def _setup(name, with_model=True):
    from cosmo_pol_amd import RadarOperator
    conf, az, el, ocube, luts, cube = _cases.radial_case(name)
    over = _cases.gen_golden.radial_case_inputs(name)[0]
    op = RadarOperator(config=over, luts=luts)
    if with_model:
        op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    return op, conf, az, el, ocube, luts


def _tol(name, k, sz, conf):
    from cosmo_pol_oracle import constants as OK
    wl = OK.Derived(conf).WAVELENGTH
    res_km = conf['radar']['radial_resolution'] / 1000.
    kdp = np.nan_to_num(1e-3 * (180.0 / np.pi) * wl * (np.abs(sz[:, 8]) + np.abs(sz[:, 10])))
    return {'KDP': RTOL * kdp, 'PHIDP': RTOL * (np.cumsum(2 * kdp) * res_km + np.pi),
            'DELTA_HV': RTOL * np.pi}.get(k, 0.0)


def _against_oracle(obs, subs, luts, conf, tag):
    oobs = scatter.radar_observables(subs, {h: _cases.as_oracle_lut(l) for h, l in luts.items()}, conf,
                                     return_sz=True)
    sz = np.nan_to_num(oobs.sz_total.astype(np.float64))
    for k in ['ZH', 'ZV', 'ZDR', 'RHOHV', 'KDP', 'ATT_H', 'ATT_V', 'DELTA_HV', 'PHIDP']:
        _cases.assert_close_nan(obs.values[k], oobs.values[k], rtol=RTOL, atol=_tol(tag, k, sz, conf), name=tag + k)
    if 'RVEL' in oobs.values:
        _cases.assert_close_nan(obs.values['RVEL'], oobs.values['RVEL'], rtol=RTOL, atol=2e-4, name=tag + 'RVEL')
    if 'DSPECTRUM' in oobs.values:
        osp = oobs.values['DSPECTRUM']
        _cases.assert_close_nan(obs.values['DSPECTRUM'], osp, rtol=2e-5, atol=1e-6 * np.nanmax(osp), name=tag + 'DSP')
    assert np.array_equal(obs.mask, oobs.mask)


@pytest.mark.parametrize('name', list(_cases.RADIAL_CASES))
def test_observables_of_oracle_subradials(golden, name):
    """get_radar_observables(oracle sub-radials) == simulate_rays bit for bit, and meets the golden / oracle."""
    from cosmo_pol_amd import radial
    g = golden('radial_' + name)
    op, conf, az, el, ocube, luts = _setup(name)
    ref = op.simulate_rays([az], [el], apply_sensitivity=False)
    sweep_forms = op._ctx.launch_forms()
    subs = beam.interpolate_radial(ocube, conf, az, el)
    before = copy.deepcopy(subs)
    obs = op.get_radar_observables(subs)
    _assert_forms(op, sweep_forms)
    for a, b in zip(subs, before):                       # never edits the caller's records
        assert np.array_equal(a.elev_profile, b.elev_profile)
        for k in b.values:
            assert np.array_equal(a.values[k], b.values[k], equal_nan=True), k
    for k in OUT:
        if k in ref:
            assert obs.values[k].dtype == ref[k].dtype
            assert np.array_equal(obs.values[k], ref[k][0], equal_nan=True), k
    assert np.array_equal(obs.mask, ref['mask'][0])
    assert np.array_equal(obs.mask, g['obs_mask'])
    for k in ['ZH', 'ZDR', 'RHOHV']:
        _cases.assert_close_nan(obs.values[k], g['obs_' + k], rtol=RTOL, name='golden:' + k)
    integ = radial.integrate_radials(subs)
    ointeg = beam.integrate_subbeams(copy.deepcopy(before))
    for k, v in ointeg.values.items():
        _cases.assert_close_nan(integ.values[k], v, rtol=1e-12, name='integ:' + k)
    _against_oracle(obs, subs, luts, conf, name + ':')
    op.close()


@pytest.mark.parametrize('name', ['c3_melt_ice', 'c4_7x7', 'q_ml_thr', 'd3_melt_ice_sub'])
def test_edited_subradials_match_oracle(name):
    """Edited records: finite QM under mask -1 / +1, NaN QM, has_melting False with QmS_v > 0, elevations 95 / -3 deg."""
    op, conf, az, el, ocube, luts = _setup(name)
    subs = beam.interpolate_radial(ocube, conf, az, el)
    n = len(subs[0].mask)
    rng = np.random.default_rng(7)
    for s, sb in enumerate(subs):
        v = sb.values
        g = rng.choice(n, size=8, replace=False)
        sb.mask = np.array(sb.mask, dtype=float)
        sb.mask[g[:2]] = -1
        sb.mask[g[2:4]] = 1
        for q in ('QR_v', 'QS_v', 'QG_v'):
            v[q][g[:4]] = np.float32(1e-4)                 # finite QM under mask +-1: scattered
        v['QR_v'][g[4]] = np.nan                           # NaN QM: no item
        v['QS_v'][g[5]] = np.nan
        sb.elev_profile = np.array(sb.elev_profile, dtype=np.float32)
        sb.elev_profile[g[6]] = np.float32(95.0)
        sb.elev_profile[g[7]] = np.float32(-3.0)
        if s == 0 and 'QmS_v' in v:
            v['QmS_v'][:] = np.where(v['QmS_v'] > 0, v['QmS_v'], 1e-4)
            sb.has_melting = False                         # dropped, whatever QmS_v holds
    obs = op.get_radar_observables(subs)
    _against_oracle(obs, subs, luts, conf, name + ':edited:')
    op.close()


def test_device_columns_on_lane_pinned_equal_host():
    """torch columns on the GPU, a lane, pinned outputs: the bits of host columns."""
    import torch
    from cosmo_pol_amd import radial
    op, conf, az, el, ocube, luts = _setup('c4_7x7')
    subs = beam.interpolate_radial(ocube, conf, az, el)
    cols = radial.subradials_to_columns(subs, op._column_names(), True)
    host = op.simulate_columns(cols)
    dev = {k: (torch.as_tensor(v).to('cuda:%d' % op.device) if k not in ('quad_pts', 'quad_weights') else v)
           for k, v in cols.items()}
    got = op.simulate_columns(dev, lane=1, pinned=True)
    op.wait(1)
    for k in OUT + ['mask']:
        if k in host:
            assert np.array_equal(got[k], host[k], equal_nan=True), k
    for k, v in dev.items():                              # inputs are read, never written
        if hasattr(v, 'cpu'):
            assert np.array_equal(v.cpu().numpy(), cols[k], equal_nan=True), k
    op.close()


def test_no_model_and_recovery_after_bad_columns():
    """An operator without a model runs get_radar_observables; calls refused before the sequence, inside it before its
    first launch (mask_sum8 with 2 n_sub > 127) and after k_columns_ingest was queued (a wind index beyond the columns)
    leave the context as it was."""
    import ctypes
    from cosmo_pol_amd import _native as N
    op, conf, az, el, ocube, luts = _setup('c3_melt_ice')
    subs = beam.interpolate_radial(ocube, conf, az, el)
    with_model = op.get_radar_observables(copy.deepcopy(subs))
    op.close()
    op, *_ = _setup('c3_melt_ice', with_model=False)
    first = op.get_radar_observables(copy.deepcopy(subs))
    for k in OUT:
        if k in with_model.values:
            assert np.array_equal(first.values[k], with_model.values[k], equal_nan=True), k
    names = op._column_names()
    keep = []

    def raw(n_vars, n_sub, n_gates=4):
        p = N.SweepParams()
        p.n_rays, p.n_gates, p.n_sub = 1, n_gates, n_sub
        p.var_u, p.var_v, p.var_w, p.var_rho = 0, 0, 0, -1
        a = np.zeros(n_sub * n_gates, dtype=np.float32)
        w = np.ones(n_sub)
        sc = np.zeros(2 * n_sub)
        ptrs = (ctypes.c_void_p * n_vars)(*([a.ctypes.data] * n_vars))
        keep.extend([a, w, sc, ptrs])
        c = N.Columns()
        c.n_vars = n_vars
        c.vals = ctypes.cast(ptrs, ctypes.c_void_p)
        c.elev = a.ctypes.data
        c.sub_w = w.ctypes.data
        c.az_sincos = sc.ctypes.data
        return p, c
    p, c = raw(1, 1)                                     # refused by cpol_run_columns' own checks
    with pytest.raises(ValueError):
        op._ctx.run_columns(p, c, N.Outputs())
    p, c = raw(len(names), 64)                           # refused inside the shared sequence, before its first launch
    m8 = np.zeros(4, dtype=np.int8)
    o = N.Outputs()
    o.mask_sum8 = m8.ctypes.data
    with pytest.raises(ValueError):
        op._ctx.run_columns(p, c, o)
    p, c = raw(len(names), 1)                            # refused after the ingest was queued
    p.simulate_doppler = 1
    p.var_u = len(names)
    zh = np.zeros(4, dtype=np.float32)
    o = N.Outputs()
    o.ZH = zh.ctypes.data
    with pytest.raises(ValueError):
        op._ctx.run_columns(p, c, o)
    with pytest.raises(ValueError):
        op.get_radar_observables([])
    again = op.get_radar_observables(copy.deepcopy(subs))
    for k in OUT:
        if k in first.values:
            assert np.array_equal(again.values[k], first.values[k], equal_nan=True), k
    op.close()


def test_bad_columns_raise_value_error():
    from cosmo_pol_amd import radial
    op, conf, az, el, ocube, luts = _setup('c3_melt_ice', with_model=False)
    subs = beam.interpolate_radial(ocube, conf, az, el)
    cols = radial.subradials_to_columns(subs, op._column_names(), True)
    bad = dict(cols)
    del bad['QmG_v']
    with pytest.raises(ValueError):
        op.simulate_columns(bad)
    op.simulate_columns(dict(cols, quad_weights=list(cols['quad_weights'])))     # a plain list is accepted
    with pytest.raises(ValueError):
        op.simulate_columns(dict(cols, quad_weights=[1.0, 2.0]))
    with pytest.raises(ValueError):
        op.simulate_columns(dict(cols, elev=cols['elev'][:, :, :-1]))
    op.close()


# ---------------------------------------------------------------- the first half: cpol_interp_subbeams

@pytest.mark.parametrize('name', list(_cases.RADIAL_CASES))
def test_interpolated_radial_vs_oracle(golden, name):
    """get_interpolated_radial == the oracle's interpolate_radial: values (melting fields included), masks, elevation,
    distance and height bit for bit, latitude / longitude to 1e-11; the central and first sub-beams == the goldens."""
    g = golden('radial_' + name)
    op, conf, az, el, ocube, luts = _setup(name)
    rad = op.get_interpolated_radial(az, el)
    subs = beam.interpolate_radial(ocube, conf, az, el)
    assert len(rad) == len(subs) == int(g['n_sub'])
    _cases.assert_radial_equals_oracle(rad, subs)
    for tag, r in (('subc_', rad[int(len(rad) / 2)]), ('subf_', rad[0])):
        for k in r.values:
            if tag + k in g.files:
                assert np.array_equal(r.values[k], g[tag + k], equal_nan=True), tag + k
        assert np.array_equal(r.mask, g[tag + 'mask'])
        assert np.array_equal(r.dist_profile, g[tag + 's'])
        assert np.array_equal(r.heights_profile, g[tag + 'h'])
        assert np.array_equal(r.elev_profile, g[tag + 'e'])
        np.testing.assert_allclose(r.lats_profile, g[tag + 'lats'], rtol=0, atol=1e-11)
        np.testing.assert_allclose(r.lons_profile, g[tag + 'lons'], rtol=0, atol=1e-11)
    op.close()


def _round_trip(op, az, el, melting):
    ref = op.simulate_rays(az, el, apply_sensitivity=False)
    sweep_forms = op._ctx.launch_forms()
    cols = op.interpolate_rays(az, el, melting=melting)
    assert ('QmS_v' in cols) == bool(melting and op.config['microphysics']['with_melting'])
    got = op.simulate_columns(cols)
    forms = _assert_forms(op, sweep_forms)
    assert set(ref) == set(got), set(ref) ^ set(got)
    for k, v in ref.items():
        if k == 'n_sub':
            assert got[k] == v
            continue
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
        assert np.array_equal(got[k], v, equal_nan=True), k
    return forms


ROUND_TRIP = ['c3_melt_ice', 'c4_7x7', 'c5_2mom', 'c5_2mom_dop2_sub', 'q_ml_dop2', 'd3_melt_ice_sub', 'q_ml_thr']


@pytest.mark.parametrize('melting', [True, False])
@pytest.mark.parametrize('name', ROUND_TRIP)
def test_round_trip_equals_sweep(name, melting):
    """simulate_columns(interpolate_rays(az, el)) == simulate_rays(az, el) for every output array: melting given
    (k_classify<true>) or diagnosed on the device after the ingest (k_classify<false>)."""
    op, conf, az, el, ocube, luts = _setup(name)
    _round_trip(op, [az, az + 0.5], [el, el], melting)
    op.close()


@pytest.mark.parametrize('melting', [True, False])
def test_round_trip_full_c2_sweep(melting):
    """The bench's C2 sweep (360 x 500 gates, one sub-beam): the single-beam gate kernel runs after the ingest."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from cosmo_pol_amd import RadarOperator
    conf, hyds, cube, luts = bench.make_inputs('c2')
    op = RadarOperator(config=conf, luts=luts)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    forms = _round_trip(op, np.arange(360.0), np.full(360, 1.0), melting)
    assert forms['gate1'] == 1
    op.close()


def test_device_export_on_lane_equals_host():
    """interpolate_rays(on_device=True) -> simulate_columns on a lane with pinned outputs: the bits of host columns."""
    op, conf, az, el, ocube, luts = _setup('c4_7x7')
    host_cols = op.interpolate_rays([az], [el], melting=True)
    dev_cols = op.interpolate_rays([az], [el], melting=True, on_device=True)
    for k, v in host_cols.items():
        d = dev_cols[k]
        d = d.cpu().numpy() if hasattr(d, 'cpu') else d
        assert np.array_equal(d, v, equal_nan=True), k
    host = op.simulate_columns(host_cols)
    got = op.simulate_columns(dev_cols, lane=1, pinned=True)
    op.wait(1)
    for k in host:
        if k != 'n_sub':
            assert np.array_equal(got[k], host[k], equal_nan=True), k
    op.close()
