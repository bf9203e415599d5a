"""Gridded composites on the GPU through the sweeps (cpol_outputs.composite): the maps of a call with keep_gates=True against
composite.compose / composite.finish of that call's own per-gate arrays, `dist`, `heights` and azimuths, exactly (NaNs
positionally equal), and the per-gate arrays, the launch forms and the gate stencils against the same call without the composite.

Cases: the golden radials c2_rsg (single beam), c3_melt_ice, c4_7x7 (49 sub-beams), c5_2mom_dop2_sub (Doppler scheme 2), seven
rays at az + 0.5 k, each with its own cube and with the planted-bad-values cube.  The grid spans the gates of a first plain call
(a few cells beyond them stay empty), the echo-top thresholds are quantiles of its values and the slab quantiles of its heights,
so that no test passes on an empty map."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_ensemble import case, load, operator
from test_gpu_histogram_sweeps import arrays, op_for, rays, _ops

pytestmark = pytest.mark.gpu

NAMES = ['c2_rsg', 'c3_melt_ice', 'c4_7x7', 'c5_2mom_dop2_sub']
CUBES = [0, 2]
FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V']


def CP():
    from cosmo_pol_amd import composite
    return composite


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() or (
        a.dtype == b.dtype and a.shape == b.shape and a.dtype == np.float32 and np.array_equal(np.isnan(a), np.isnan(b))
        and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32)))


def same_gates(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def plain_run(name, cube):
    op = op_for(name, cube)
    az, el = rays(name)
    res = arrays(op.simulate_rays(az, el))
    return res, op._ctx.launch_forms()


def finite_quantiles(v, qs):
    v = np.asarray(v, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    return [0.0] * len(qs) if v.size == 0 else [float(x) for x in np.quantile(v, qs)]


def spec_for(plain, az, products=('max', 'lowest', 'echo_top'), slab=True, fields=FIELDS, n=(9, 7)):
    """A grid over the gates of `plain` (non-uniform, one ring of cells beyond them), thresholds and slab from the data."""
    c = CP()
    rs, rc = c.ray_tables(az)
    d = np.asarray(plain['dist'], dtype=np.float64)
    x, y = d * rs[:, None], d * rc[:, None]

    def axis(v, cells):
        lo, hi = float(np.nanmin(v)), float(np.nanmax(v))
        pad = 0.1 * (hi - lo) + 1.0
        return (lo - pad) + (hi - lo + 2 * pad) * (np.arange(cells + 1) / cells) ** 1.3
    kw = {}
    if 'echo_top' in products:
        kw['thresholds'] = {k: finite_quantiles(plain[k], [0.3, 0.6]) if k != 'KDP' else finite_quantiles(plain[k], [0.5]) for k in fields}
    if slab:
        kw['height_range'] = tuple(finite_quantiles(plain['heights'], [0.05, 0.9]))
    return c.Composite(fields, axis(x, n[0]), axis(y, n[1]), products=products, **kw)


def maps_of(res):
    w = res['composite']
    return {'values': {k: {p: np.array(a) for p, a in v.items()} for k, v in w['values'].items()},
            'count': {k: np.array(a) for k, a in w['count'].items()}}


def rule(spec, sweeps, rpb=0):
    """composite.compose over [(per-gate arrays, azimuths)] in turn, finished."""
    c = CP()
    state = None
    for gates, az in sweeps:
        state = c.compose(spec, {k: gates[k] for k in spec.fields}, gates['dist'], gates['heights'], az, state=state, rays_per_block=rpb)
    return c.finish(state)


def assert_maps(got, want, spec, tag, not_empty=True):
    assert sorted(got['values']) == sorted(spec.fields) == sorted(got['count']), tag
    for k in spec.fields:
        assert list(got['values'][k]) == spec.planes(k), (tag, k)
        for p in spec.planes(k):
            assert same(got['values'][k][p], want['values'][k][p]), (tag, k, p)
        assert same(got['count'][k], want['count'][k]), (tag, k, 'count')
    n = got['count'][spec.fields[0]]
    print('%s: %d gates counted for %s in %d of %d cells' % (tag, int(n.sum()), spec.fields[0], int((n > 0).sum()), n.size))
    if not_empty:
        assert int((n > 0).sum()) >= 3 and int((n == 0).sum()) >= 1, (tag, n.tolist())


@pytest.mark.parametrize('cube', CUBES)
@pytest.mark.parametrize('name', NAMES)
def test_maps_of_the_rule(name, cube):
    op = op_for(name, cube)
    az, el = rays(name)
    plain, forms = plain_run(name, cube)
    for i, (products, slab) in enumerate(((('max', 'lowest', 'echo_top'), True), (('max',), False))):
        spec = spec_for(plain, az, products, slab)
        tag = '%s/cube %d/%s' % (name, cube, '+'.join(products))
        res = op.simulate_rays_composite(az, el, spec, keep_gates=True)
        got, gates = maps_of(res), arrays(res)
        assert op._ctx.launch_forms() == forms, tag
        for k, v in plain.items():                       # the per-gate arrays are those of the call without the composite
            assert same_gates(gates[k], v), (tag, 'per-gate', k)
        assert_maps(got, rule(spec, [(gates, az)]), spec, tag)
        if i == 0:
            # per ray, and without the gates
            per_ray = op.simulate_rays_composite(az, el, spec, keep_gates=True, rays_per_block=1)
            assert_maps(maps_of(per_ray), rule(spec, [(arrays(per_ray), az)], rpb=1), spec, tag + '/per ray', not_empty=False)
            assert np.array_equal(maps_of(per_ray)['count']['ZH'].sum(axis=0, keepdims=True), got['count']['ZH'])
            only = op.simulate_rays_composite(az, el, spec)
            for k in FIELDS + ['RVEL', 'mask', 'mask_sum8', 'model_vars']:
                assert k not in only, k
            assert_maps(maps_of(only), got, spec, tag + '/maps only')
            assert np.array_equal(only['composite']['x_edges'], spec.x_edges) and np.array_equal(only['composite']['y_edges'], spec.y_edges)


def test_stencils_and_forms_are_left_alone():
    """Five sweeps of one geometry with the composite and five of another without: the same stencil forms (full, recording,
    replay ...) and launch forms sweep by sweep, and every sweep's arrays those of the plain call."""
    name = 'c2_rsg'
    conf, luts, cubes, _, _ = case(name)
    az, el = rays(name)
    spec = spec_for(plain_run(name, 2)[0], az)
    seen = {}
    for with_comp in (False, True):
        op = operator(conf, luts)
        load(op, cubes[2])
        st, forms, out = [], [], []
        for i in range(5):
            res = op.simulate_rays_composite(az, el, spec, keep_gates=True) if with_comp else op.simulate_rays(az, el)
            out.append((arrays(res), maps_of(res) if with_comp else None))
            st.append(op.stencil_state()['form'])
            forms.append(op._ctx.launch_forms())
        seen[with_comp] = (st, forms, out)
        op.close()
    print('stencil forms without / with the composite:', seen[False][0], seen[True][0])
    assert seen[False][0] == seen[True][0] and seen[True][0][-1] == 2
    assert seen[False][1] == seen[True][1]
    for i in range(5):
        for k, v in seen[False][2][i][0].items():
            assert same_gates(seen[True][2][i][0][k], v), (i, k)
        assert_maps(seen[True][2][i][1], rule(spec, [(seen[True][2][i][0], az)]), spec, 'sweep %d' % i)


def captured(op, az, el, spec, **kw):
    """simulate_rays_composite, and copies of the cpol_sweep_params / cpol_ray_tables_t it handed to Context.run_sweep"""
    from cosmo_pol_amd import _native as N
    ctx, seen = op._ctx, {}
    orig = ctx.run_sweep

    def spy(p, t, o):
        seen['p'], seen['t'] = N.SweepParams.from_buffer_copy(p), N.RayTables.from_buffer_copy(t)
        return orig(p, t, o)
    ctx.run_sweep = spy
    try:
        res = op.simulate_rays_composite(az, el, spec, **kw)
    finally:
        del ctx.run_sweep
    return res, seen['p'], seen['t']


def direct(op, spec, az, want, p, t, mode, change=None, outputs=None, entry='run_sweep'):
    """One cpol_run_sweep with a cpol_composite of its own in output mode `mode` -> the maps (mode 1: torch tensors)."""
    import torch
    from cosmo_pol_amd import _native as N
    c, keep = N.Context.composite_struct(spec, azimuths=az)
    vals, cnt = {}, None
    n_fields = len(spec.fields)
    for i, k in enumerate(spec.fields):
        sh = (want['count'][k].shape[0], len(spec.planes(k))) + want['count'][k].shape[1:]
        if mode == 1:
            vals[k] = torch.full(sh, 77.0, dtype=torch.float32, device='cuda')
            c.values[CP().FIELDS.index(k)] = vals[k].data_ptr()
        else:
            vals[k] = np.full(sh, 77.0, dtype=np.float32)
            c.values[CP().FIELDS.index(k)] = vals[k].ctypes.data
    sh = (want['count'][spec.fields[0]].shape[0], n_fields) + want['count'][spec.fields[0]].shape[1:]
    if mode == 1:
        cnt = torch.full(sh, 77, dtype=torch.int64, device='cuda')
        c.count = cnt.data_ptr()
    else:
        cnt = np.full(sh, 77, dtype=np.uint64)
        c.count = cnt.ctypes.data
    if change:
        keep.append(change(c))
    o = N.Outputs()
    o.composite = C.pointer(c)
    if outputs:
        keep.append(outputs(o))
    q = N.SweepParams.from_buffer_copy(p)
    q.outputs_on_device = mode
    if entry == 'run_columns':
        op._ctx.run_columns(q, N.Columns(), o)
    else:
        op._ctx.run_sweep(q, t, o)
    op.wait()
    del keep
    if mode == 1:
        vals = {k: v.cpu().numpy() for k, v in vals.items()}
        cnt = cnt.cpu().numpy().view(np.uint64)
    return {'values': {k: {p_: vals[k][:, j] for j, p_ in enumerate(spec.planes(k))} for k in spec.fields},
            'count': {k: cnt[:, i] for i, k in enumerate(spec.fields)}}


@pytest.mark.parametrize('name', ['c2_rsg', 'c5_2mom_dop2_sub'])
def test_output_modes(name):
    """Blocking host buffers, device pointers and page-locked buffers (waited for, and pinned=True + wait) carry the same maps."""
    import torch
    op = op_for(name, 2)
    az, el = rays(name)
    spec = spec_for(plain_run(name, 2)[0], az)
    locked, p, t = captured(op, az, el, spec, keep_gates=True)
    want = maps_of(locked)
    assert_maps(want, rule(spec, [(arrays(locked), az)]), spec, name + '/page-locked')
    lazy = op.simulate_rays_composite(az, el, spec, pinned=True)
    op.wait()
    assert_maps(maps_of(lazy), want, spec, name + '/pinned')
    assert_maps(direct(op, spec, az, want, p, t, 0), want, spec, name + '/blocking')
    assert_maps(direct(op, spec, az, want, p, t, 1), want, spec, name + '/device')
    # ... and through the operator: device_outputs['composite'], a pass of two calls (max, min and echo tops of the same sweep
    # twice are those of one; the counts double)
    dv = {k: torch.full((want['count'][k].shape[0], len(spec.planes(k))) + want['count'][k].shape[1:], 77.0, dtype=torch.float32, device='cuda')
          for k in spec.fields}
    dc = torch.full((want['count']['ZH'].shape[0], len(spec.fields)) + want['count']['ZH'].shape[1:], 77, dtype=torch.int64, device='cuda')
    ptrs = {'composite': {'values': {k: a.data_ptr() for k, a in dv.items()}, 'count': dc.data_ptr()}}
    op.simulate_rays_composite(az, el, spec, phase=1, device_outputs=ptrs)
    op.wait()
    assert (dc == 77).all().item() and all((a == 77.0).all().item() for a in dv.values())       # nothing is written before the finish
    op.simulate_rays_composite(az, el, spec, phase=2, device_outputs=ptrs)
    op.wait()
    for i, k in enumerate(spec.fields):
        assert np.array_equal(dc.cpu().numpy().view(np.uint64)[:, i], 2 * want['count'][k]), k
        for j, q in enumerate(spec.planes(k)):
            assert same(dv[k].cpu().numpy()[:, j], want['values'][k][q]), (k, q)


def test_scans():
    """A 3-elevation get_PPI_composite against the rule on the three sweeps, and per_sweep=True."""
    name = 'c2_rsg'
    op = op_for(name, 0, lanes=2)
    az, _ = rays(name)
    elevations = [4.0, 5.0, 6.0]
    spec = spec_for(plain_run(name, 0)[0], az)
    kept = op.get_PPI_composite(elevations, spec, azimuths=az, keep_gates=True)
    assert len(kept['sweeps']) == 3 and 'composite' not in kept['sweeps'][0]
    want = rule(spec, [(arrays(s), az) for s in kept['sweeps']])
    assert_maps(maps_of(kept), want, spec, 'volume')
    # cut differently: 1 + 2 calls through the operator give the same bits
    op.simulate_rays_composite(az, np.full(len(az), 4.0), spec, phase=1)
    op.simulate_rays_composite(az, np.full(len(az), 6.0), spec, phase=0)
    last = op.simulate_rays_composite(az, np.full(len(az), 5.0), spec, phase=2)
    assert_maps(maps_of(last), want, spec, 'volume in another order')
    volume = op.get_PPI_composite(elevations, spec, azimuths=az)
    assert 'ZH' not in volume['sweeps'][0]
    assert_maps(maps_of(volume), want, spec, 'volume, maps only')
    per_sweep = op.get_PPI_composite(elevations, spec, azimuths=az, per_sweep=True, keep_gates=True)
    assert len(per_sweep) == 3
    for i in range(3):
        assert_maps(maps_of(per_sweep[i]), rule(spec, [(arrays(per_sweep[i]), az)]), spec, 'sweep %d' % i)
    assert not same(maps_of(per_sweep[0])['values']['ZH']['height_of_max'], maps_of(per_sweep[2])['values']['ZH']['height_of_max'])


def test_ensemble():
    name = 'c4_7x7'
    op, _, _ = E.ensemble_operator(name)
    az, el = rays(name)
    first = arrays(op.simulate_rays_ensemble(az, el))
    spec = spec_for(first, az)
    kept = op.simulate_rays_ensemble_composite(az, el, spec, keep_gates=True)
    got, gates = maps_of(kept), arrays(kept)
    assert gates['ZH'].shape[0] == 3 and gates['heights'].shape == gates['ZH'].shape[1:]
    for k in FIELDS:
        assert same_gates(gates[k], first[k]), k
    assert_maps(got, rule(spec, [(gates, az)], rpb=len(az)), spec, 'ensemble')
    assert got['count']['ZH'].shape[0] == 3
    only = op.simulate_rays_ensemble_composite(az, el, spec)
    assert 'ZH' not in only
    assert_maps(maps_of(only), got, spec, 'ensemble, maps only')
    whole = maps_of(op.simulate_rays_ensemble_composite(az, el, spec, per_member=False))
    assert_maps(whole, rule(spec, [(gates, az)]), spec, 'ensemble, one map')
    for m in range(3):
        op.select_member(m)
        alone = maps_of(op.simulate_rays_composite(az, el, spec))
        for k in spec.fields:
            for q in spec.planes(k):
                assert same(got['values'][k][q][m:m + 1], alone['values'][k][q]), (m, k, q)
    op.select_member(0)
    assert not same(got['values']['ZH']['max'][0], got['values']['ZH']['max'][1])
    # the member list cut into chunks: the same maps
    op.sequence_memory_budget = 1
    cut = op.simulate_rays_ensemble_composite(az, el, spec)
    cut_whole = op.simulate_rays_ensemble_composite(az, el, spec, per_member=False)
    op.sequence_memory_budget = None
    assert_maps(maps_of(cut), got, spec, 'ensemble in chunks')
    assert_maps(maps_of(cut_whole), whole, spec, 'ensemble in chunks, one map')
    op.close()


def test_time_blend():
    import test_gpu_timed as T
    name = 'c4_7x7'
    op, _, _ = T.series_operator(name)
    az, el = rays(name)
    plain = T.arrays(op.simulate_rays_at(az, el, 200.0))
    spec = spec_for(plain, az)
    res = op.simulate_rays_at_composite(az, el, 200.0, spec, keep_gates=True)
    got, gates = maps_of(res), arrays(res)
    for k, v in plain.items():
        assert same_gates(gates[k], v), k
    assert_maps(got, rule(spec, [(gates, az)]), spec, 'timed')
    only = op.simulate_rays_at_composite(az, el, 200.0, spec)
    assert 'ZH' not in only
    assert_maps(maps_of(only), got, spec, 'timed, maps only')
    op.close()


def test_refusals_leave_the_pass_and_the_context_usable():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import histogram as HG
    from cosmo_pol_amd import superob as SO
    c = CP()
    name = 'c2_rsg'
    op = op_for(name, 2)
    az, el = rays(name)
    spec = spec_for(plain_run(name, 2)[0], az)
    good, p, t = captured(op, az, el, spec)
    good = maps_of(good)
    # a pass is open while the refusals come
    op.simulate_rays_composite(az, el, spec, phase=1)
    op.wait()

    def call(change=None, outputs=None, entry='run_sweep', phase=2):
        def both(s):
            s.phase = phase
            return change(s) if change else None
        return direct(op, spec, az, good, p, t, 0, change=both, outputs=outputs, entry=entry)
    for word, change in (('phase', lambda s: setattr(s, 'phase', 4)), ('rays_per_block', lambda s: setattr(s, 'rays_per_block', 3)),
                         ('RVEL', lambda s: setattr(s, 'fields', s.fields | 1 << 9)), ('products', lambda s: setattr(s, 'products', 0)),
                         ('products', lambda s: setattr(s, 'products', 15)), ('ray_sin', lambda s: setattr(s, 'ray_sin', None)),
                         ('ray_sin', lambda s: setattr(s, 'ray_cos', None)), ('h_lo < h_hi', lambda s: setattr(s, 'h_hi', s.h_lo)),
                         ('differ', lambda s: setattr(s, 'use_slab', 0)), ('differ', lambda s: setattr(s, 'fields', 1)),
                         ('count', lambda s: setattr(s, 'count', None))):
        with pytest.raises(ValueError, match=word):
            call(change)
    too_many = lambda s: s.n_thresholds.__setitem__(0, 5)      # noqa: E731
    with pytest.raises(ValueError, match='thresholds'):
        call(too_many)
    with pytest.raises(ValueError, match='NaN'):
        call(lambda s: s.thresholds[0].__setitem__(0, np.nan))
    # not together with another product; not through cpol_run_columns; no spaceborne call
    so = N.Superob()
    so.ray_window, so.gate_window, so.min_valid_fraction = 3, 5, 0.5
    zh = np.zeros(SO.shape(len(az), len(op.constants.RANGE_RADAR), SO.Superob(3, 5, 0.5)), dtype=np.float32)
    so.ZH = zh.ctypes.data
    hs, hkeep = N.Context.histogram_struct(HG.Histogram({'ZH': [1.0, 2.0]}))
    ms, sm = N.MemberStats(), N.SpectrumMoments()
    for other, s in (('superob', so), ('histogram', hs), ('member_stats', ms), ('spectrum_moments', sm)):
        with pytest.raises(ValueError, match='cpol_composite: not together'):
            call(outputs=lambda o, other=other, s=s: setattr(o, other, C.pointer(s)))
    with pytest.raises(ValueError, match='composite'):
        call(entry='run_columns')
    site = np.zeros((len(az), 3))
    t_site = N.RayTables.from_buffer_copy(t)
    t_site.site = site.ctypes.data
    with pytest.raises(ValueError, match='spaceborne'):
        direct(op, spec, az, good, p, t_site, 0, change=lambda s: setattr(s, 'phase', 2))
    # nothing was queued and the pass is as it was: it finishes with the bits of one sweep folded twice
    twice = call()
    for k in spec.fields:
        assert np.array_equal(twice['count'][k], 2 * good['count'][k]), k
        for q in spec.planes(k):
            assert same(twice['values'][k][q], good['values'][k][q]), (k, q)
    with pytest.raises(ValueError, match='no pass open'):
        call(phase=0)
    assert_maps(call(phase=3), good, spec, 'after the refusals')
    # the operator's own refusals
    with pytest.raises(ValueError):
        op.simulate_rays_composite(az, el, {'ZH': [1.0, 2.0]})
    with pytest.raises(ValueError):
        op.simulate_rays_composite(az, el, spec, rays_per_block=3)
    with pytest.raises(ValueError):
        c.Composite(['RVEL'], [0.0, 1.0], [0.0, 1.0])
    op.distributed = True
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_composite(az, el, spec)
        with pytest.raises(NotImplementedError):
            op.get_PPI_composite([4.0], spec, azimuths=az)
    finally:
        op.distributed = False
    high = op.config
    low = op.config
    high['radar']['coords'] = [46.5, 7.5, 400000.]
    op.config = high
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_composite(az, el, spec)
    finally:
        op.config = low
    assert_maps(maps_of(op.simulate_rays_composite(az, el, spec)), good, spec, 'after the operator refusals')
