"""Time-interpolated scans on the GPU (cpol_run_sweep_members with cpol_ray_tables_t.time_blend, k_interp_timed): every output
array of a timed sweep against simulate_rays of a fresh operator loaded -- through load_model_arrays -- with the cube blended on
the host by timeline.blend_states, bit for bit.  Three states: the case's cube, perturbed(cube, 101) and
perturbed(cube, 202, plant=True), at the times SERIES."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
import test_gpu_seam as S
from test_gpu_ensemble import FIELDS, GEOM, case, load, operator, perturbed

pytestmark = pytest.mark.gpu

CASES = list(S.ROUND_TRIP) + ['c2_rsg']
SERIES = [0.0, 600.0, 1500.0]
W_THIRD = np.float32(np.float64(200.0) / np.float64(600.0))      # the weight of t = 200 s: not a dyadic fraction


def series_operator(name, output_variables='only_radar', **kw):
    from cosmo_pol_amd import RadarOperator
    conf, luts, cubes, az, el = case(name)
    op = RadarOperator(config=copy.deepcopy(conf), luts=luts, output_variables=output_variables, **kw)
    op.load_model_series([c['data'] for c in cubes], SERIES, cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    assert op.n_members == 3 and np.array_equal(op.series_times, SERIES)
    return op, az, el


def arrays(res):
    return {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}


@functools.lru_cache(maxsize=None)
def blended(name, lo, w_bits, output_variables='only_radar', plant=True):
    """simulate_rays (the case's two rays) of a fresh operator loaded with blend_states(state lo, state lo + 1, w)."""
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_amd import timeline as TL
    conf, luts, cubes, az, el = case(name)
    w = np.array([w_bits], dtype=np.uint32).view(np.float32)[0]
    hi = cubes[lo + 1] if (plant or lo + 1 != 2) else perturbed(cubes[0], 202)
    data = TL.blend_states(cubes[lo]['data'], hi['data'], w)
    for v in data.values():
        assert v.dtype == np.float32
    op = RadarOperator(config=copy.deepcopy(conf), luts=luts, output_variables=output_variables)
    load(op, dict(cubes[0], data=data))
    out = arrays(op.simulate_rays(az, el))
    op.close()
    return out


def bits(w):
    return int(np.array([w], dtype=np.float32).view(np.uint32)[0])


def assert_same(got, ref, tag, rows=None, ref_rows=None, keys=FIELDS + GEOM):
    """every output array (or its rows `rows` against the reference's `ref_rows`): dtype, shape, every gate"""
    n = 0
    for k in keys:
        assert (k in got) == (k in ref), (tag, k)
        if k not in ref:
            continue
        a = got[k] if rows is None else got[k][rows]
        b = ref[k] if ref_rows is None else ref[k][ref_rows]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, k, a.dtype, b.dtype, a.shape, b.shape)
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        print('%s %s: %d of %d values differ' % (tag, k, int((~same).sum()), same.size))
        assert np.array_equal(a, b, equal_nan=True), (tag, k, int((~same).sum()))
        n += 1
    return n


def differs(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


@pytest.mark.parametrize('name', CASES)
def test_one_weight_for_the_scan(name):
    op, az, el = series_operator(name)
    n_vars = len(op._staged_vars)
    print('%s: n_vars = %d, n_vars %% 4 = %d (%s)' % (name, n_vars, n_vars % 4,
                                                      'groups of four only' if n_vars % 4 == 0 else 'groups and a tail'))
    for t, w in ((150.0, np.float32(0.25)), (200.0, W_THIRD)):
        got = arrays(op.simulate_rays_at(az, el, t))
        forms = op._ctx.launch_forms()
        assert forms['interp_classify'] == 0 and forms['graph_replayed'] == 0, forms
        ref = blended(name, 0, bits(w))
        n = assert_same(got, ref, '%s/w=%r' % (name, float(w)))
        assert n >= 14, n                                  # the 9 polarimetric fields, the mask and the 4 gate coordinates at least
        assert np.isfinite(got['ZH']).sum() > 0
        states = E.alone(name)
        assert differs(got['ZH'], states[0][0]['ZH']) > 0 and differs(got['ZH'], states[1][0]['ZH']) > 0
    assert int(op._member) == 0
    op.close()


@pytest.mark.parametrize('name', ['c4_7x7', 'c2_rsg'])
def test_per_ray_brackets_and_weights_in_one_call(name):
    op, az, el = series_operator(name)
    az4, el4 = np.concatenate([az, az]), np.concatenate([el, el])
    times = [150.0, 600.0 + 0.625 * 900.0, 0.0, 1500.0]    # (lo 0, w 0.25), (lo 1, w 0.625), state 0, the last state
    from cosmo_pol_amd import timeline as TL
    lo, w = TL.bracket(SERIES, times)
    assert lo.tolist() == [0, 1, 0, 2] and w.tolist() == [0.25, 0.625, 0.0, 0.0]
    got = arrays(op.simulate_rays_at(az4, el4, times))
    states = E.alone(name)
    assert_same(got, blended(name, 0, bits(0.25)), name + '/ray 0', rows=slice(0, 1), ref_rows=slice(0, 1))
    assert_same(got, blended(name, 1, bits(0.625)), name + '/ray 1', rows=slice(1, 2), ref_rows=slice(1, 2))
    assert_same(got, states[0][0], name + '/ray 2 = state 0', rows=slice(2, 3), ref_rows=slice(0, 1))
    assert_same(got, states[2][0], name + '/ray 3 = state 2', rows=slice(3, 4), ref_rows=slice(1, 2))
    # the planted NaN / -9999 / negative values of state 2 reach the ray that blends states 1 and 2
    clean = blended(name, 1, bits(0.625), plant=False)
    assert differs(got['mask'][1], clean['mask'][1]) > 0, 'the planted values of state 2 did not reach the blended ray'
    assert differs(got['ZH'][1], clean['ZH'][1]) > 0
    op.close()


@pytest.mark.parametrize('name', ['c2_rsg', 'c4_7x7'])
def test_model_variables(name):
    op, az, el = series_operator(name, output_variables='all')
    got = arrays(op.simulate_rays_at(az, el, 150.0))
    ref = blended(name, 0, bits(0.25), output_variables='all')
    assert got['model_vars'].shape == (len(op._staged_vars), len(az), ref['ZH'].shape[1])
    assert_same(got, ref, name + '/all', keys=FIELDS + GEOM + ['model_vars'])
    assert np.isfinite(got['model_vars']).sum() > 0
    op.close()


def test_lanes_and_the_ordinary_calls_around_a_timed_one():
    name = 'c4_7x7'
    op, az, el = series_operator(name)
    op.select_member(1)
    before = arrays(op.simulate_rays(az, el))
    assert differs(before['ZH'], E.alone(name)[0][0]['ZH']) > 0            # (really member 1)
    r0 = arrays(op.simulate_rays_at(az, el, 200.0))
    r1 = op.simulate_rays_at(az, el, 200.0, lane=1, pinned=True)
    op.wait(1)
    r1 = arrays(r1)
    assert_same(r1, r0, 'lane 1 (pinned) = lane 0')
    assert_same(r0, blended(name, 0, bits(W_THIRD)), 'lane 0 = blended cube')
    after = arrays(op.simulate_rays(az, el))
    assert_same(after, before, 'simulate_rays after = before')
    assert_same(arrays(op.simulate_rays(az, el, lane=1)), before, 'simulate_rays on lane 1')
    assert int(op._member) == 1
    op.close()


def test_scans_are_their_rays():
    name = 'c3_melt_ice'
    op, az, el = series_operator(name)
    a, e = float(az[0]), float(el[0])
    azs = np.array([a, a + 0.5, a + 1.0])
    ppi = op.get_PPI_at([e, e + 1.0], [150.0, 1162.5], azimuths=azs)
    assert ppi.nsweeps == 2 and ppi.scan_type == 'ppi'
    for i, (ee, t) in enumerate(((e, 150.0), (e + 1.0, 1162.5))):
        ref = op.simulate_rays_at(azs, np.full(3, ee), t)
        sw = ppi.raw[i]
        for k in ('ZH', 'ZDR', 'KDP', 'RHOHV', 'RVEL'):
            assert np.array_equal(sw['fields'][k], ref[k], equal_nan=True), (i, k)
        for k in ('mask', 'lats', 'lons', 'dist', 'heights'):
            assert np.array_equal(sw[k], ref[k], equal_nan=True), (i, k)
    # one array of times per sweep
    per_ray = [np.array([150.0, 200.0, 0.0]), np.array([1500.0, 700.0, 600.0])]
    ppi2 = op.get_PPI_at([e, e + 1.0], per_ray, azimuths=azs)
    for i, ee in enumerate((e, e + 1.0)):
        ref = op.simulate_rays_at(azs, np.full(3, ee), per_ray[i])
        assert np.array_equal(ppi2.raw[i]['fields']['ZH'], ref['ZH'], equal_nan=True), i
    els = np.array([e, e + 0.5])
    rhi = op.get_RHI_at([a], [200.0], elevations=els)
    ref = op.simulate_rays_at(np.full(2, a), els, 200.0)
    assert rhi.nsweeps == 1 and rhi.scan_type == 'rhi'
    for k in ('ZH', 'ZV', 'PHIDP'):
        assert np.array_equal(rhi.raw[0]['fields'][k], ref[k], equal_nan=True), k
    assert np.isfinite(ref['ZH']).sum() > 0
    op.close()


def test_launch_forms():
    op, az, el = series_operator('c2_rsg')
    op.simulate_rays_at(az, el, 150.0)
    f = op._ctx.launch_forms()
    assert f['n_sub'] == 1 and f['gate1'] == 1 and f['interp_classify'] == 0 and f['graph_replayed'] == 0, f
    op.close()
    op, az, el = series_operator('c4_7x7')
    op.simulate_rays_at(az, el, 150.0)
    f = op._ctx.launch_forms()
    assert f['n_sub'] == 49 and f['gate1'] == 0 and f['interp_classify'] == 0 and f['graph_replayed'] == 0, f
    op.close()


def test_refused_library_calls_leave_the_context_usable():
    from cosmo_pol_amd import _native as N
    name = 'c4_7x7'
    op, az, el = series_operator(name)
    ctx = op._ctx
    seen = {}
    plain = ctx.run_sweep_members

    def spy(p, t, members, o):
        seen['args'] = (p, N.RayTables.from_buffer_copy(t), np.array(members, dtype=np.int32), o)
        return plain(p, t, members, o)
    ctx.run_sweep_members = spy
    first = op.simulate_rays_at(az, el, 150.0)             # (kept: the output struct points into its block)
    ctx.run_sweep_members = plain
    good = arrays(first)
    p, t, members, o = seen['args']
    assert t.time_blend == 1 and members.tolist() == [0, 1]
    n = len(az)

    def call(weights, states, members=members, entry='members'):
        q = N.RayTables.from_buffer_copy(t)
        wv = np.ascontiguousarray(weights, dtype=np.float32)
        sv = np.ascontiguousarray(states, dtype=np.int32)
        q.ray_weight, q.ray_state = wv.ctypes.data, sv.ctypes.data
        if entry == 'members':
            return ctx.lib.cpol_run_sweep_members(ctx.h, C.byref(p), C.byref(q), members.ctypes.data_as(C.c_void_p), len(members),
                                                  C.byref(o))
        return ctx.lib.cpol_run_sweep(ctx.h, C.byref(p), C.byref(q), C.byref(o))

    refused = [
        ('a weight of 1.0', call([0.25] + [1.0] * (n - 1), [0] * n)),
        ('a NaN weight', call([np.nan] + [0.25] * (n - 1), [0] * n)),
        ('a negative weight', call([-0.25] * n, [0] * n)),
        ('the later state out of range', call([0.25] * n, [0] * (n - 1) + [1])),
        ('the earlier state out of range', call([0.0] * n, [0] * (n - 1) + [2])),
        ('a negative state', call([0.0] * n, [-1] * n)),
        ('time_blend in cpol_run_sweep', call([0.25] * n, [0] * n, entry='sweep')),
    ]
    for what, rc in refused:
        assert rc == N.ERR_ARG, (what, rc)
    # the last state alone (w = 0) is no error ...
    assert call([0.0] * n, [1] * n) == 0
    ctx.synchronize()
    # ... and a good call gives the first one's bits
    assert_same(arrays(op.simulate_rays_at(az, el, 150.0)), good, 'after the refusals')
    assert_same(good, blended(name, 0, bits(0.25)), 'the first call')
    op.close()


def test_refused_operator_calls():
    name = 'c2_rsg'
    op, az, el = series_operator(name)
    for t in (-1.0, 1500.5, np.nan):
        with pytest.raises(ValueError, match='outside the series'):
            op.simulate_rays_at(az, el, t)
    with pytest.raises(ValueError):
        op.simulate_rays_at(az, el, [0.0, 1.0, 2.0])       # neither one time nor one per ray
    with pytest.raises(ValueError):
        op.get_PPI_at([1.0, 2.0], [0.0], azimuths=az)       # one entry per sweep
    conf = op._RadarOperator__config
    op.distributed = True
    with pytest.raises(NotImplementedError, match='process group'):
        op.simulate_rays_at(az, el, 10.0)
    op.distributed = False
    conf['refraction']['scheme'] = 2
    with pytest.raises(NotImplementedError, match='refraction'):
        op.get_PPI_at([1.0], [10.0], azimuths=az)
    conf['refraction']['scheme'] = 1
    alt = conf['radar']['coords'][2]
    conf['radar']['coords'][2] = 400000.0
    with pytest.raises(NotImplementedError, match='spaceborne'):
        op.get_RHI_at([0.0], [10.0], elevations=el)
    conf['radar']['coords'][2] = alt
    ok = arrays(op.simulate_rays_at(az, el, 10.0))           # (the operator is as it was)
    assert np.isfinite(ok['ZH']).sum() > 0
    # whatever drops the members drops the series
    cubes = case(name)[2]
    load(op, cubes[0])
    assert op.series_times is None and op.n_members == 1
    with pytest.raises(ValueError, match='no series'):
        op.simulate_rays_at(az, el, 10.0)
    # dicts of arrays carry no time of their own; a series must increase
    with pytest.raises(ValueError, match='no time'):
        op.load_model_series([c['data'] for c in cubes], None, cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    with pytest.raises(ValueError, match='increase'):
        op.load_model_series([c['data'] for c in cubes], [0.0, 5.0, 5.0], cubes[0]['zlevels'], cubes[0]['proj_info'],
                             cubes[0]['resolution'])
    with pytest.raises(AttributeError):
        op.series_times = [1.0, 2.0]
    op.close()
