"""Sweep histograms on the GPU through the sweeps (cpol_outputs.histogram): the counts of a call with keep_gates=True against
histogram.count of that call's own per-gate arrays, exactly, and the per-gate arrays, the launch forms and the gate stencils
against the same call without the histogram.

Cases: the golden radials c2_rsg (single beam), c3_melt_ice, c4_7x7 (49 sub-beams), c5_2mom_dop2_sub (Doppler scheme 2), seven
rays at az + 0.5 k, each with its own cube and with the planted-bad-values cube.  The edges are made from the data (the
deciles of a first plain call's counting values) and from a hand-set dB list, so that no test passes on an empty table."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

NAMES = ['c2_rsg', 'c3_melt_ice', 'c4_7x7', 'c5_2mom_dop2_sub']
CUBES = [0, 2]
N_RAYS = 7
GATE_FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL']
_ops = {}


def HG():
    from cosmo_pol_amd import histogram
    return histogram


@functools.lru_cache(maxsize=None)
def rays(name, n=N_RAYS, shift=0.0):
    _, _, _, az, el = case(name)
    return az[0] + shift + 0.5 * np.arange(n), np.full(n, el[0])


def op_for(name, cube=0, **kw):
    key = (name, cube, tuple(sorted(kw.items())))
    if key not in _ops:
        conf, luts, cubes, _, _ = case(name)
        if 'output_variables' in kw:
            from cosmo_pol_amd import RadarOperator
            op = RadarOperator(config=copy.deepcopy(conf), luts=luts, **kw)
        else:
            op = operator(conf, luts, **kw)
        load(op, cubes[cube])
        _ops[key] = op
    return _ops[key]


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def arrays(res):
    return {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}


def counts_of(res):
    return {k: np.array(v) for k, v in res['histogram']['counts'].items()}


def decile_edges(values, dt):
    """The interior edges at the deciles of the counting values, deduplicated after rounding to the field's type (at least two)."""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    if v.size == 0:
        return np.array([0.0, 1.0])
    e = np.unique(np.quantile(v, np.arange(1, 10) / 10.0).astype(dt)).astype(np.float64)
    if e.size < 2:
        e = np.array([e[0], e[0] + max(1.0, abs(e[0]))])
    return e


@functools.lru_cache(maxsize=None)
def plain_run(name, cube):
    op = op_for(name, cube)
    az, el = rays(name)
    res = arrays(op.simulate_rays(az, el))
    return res, op._ctx.launch_forms()


def specs_for(name, cube, ordinate='heights'):
    """[the histogram with edges at the deciles of the data, the one with hand-set dB edges] over every field the case has."""
    H = HG()
    plain, _ = plain_run(name, cube)
    fields = [k for k in GATE_FIELDS if k in plain]
    data = {k: decile_edges(plain[k], H.dtype_of(k)) for k in fields}
    hand = {k: (np.arange(-20.0, 21.0, 2.5) if k == 'RVEL' else H.db_edges(-40, 60, 4)) for k in fields}
    oe = None if ordinate is None else decile_edges(plain[ordinate], H.dtype_of(ordinate))
    return [H.Histogram(data, ordinate=ordinate, ordinate_edges=oe), H.Histogram(hand, ordinate=ordinate, ordinate_edges=oe)], fields


def assert_counts(got, res, spec, tag, rpb=0, not_empty=True):
    """the counts of a result == histogram.count of its own per-gate arrays; (with edges from the data) not on an empty table"""
    H = HG()
    want = H.count(res, spec, rpb)
    assert sorted(got) == sorted(spec.fields), tag
    for k in spec.fields:
        assert same(got[k], want[k]), (tag, k, got[k].shape, want[k].shape, int(got[k].sum()), int(want[k].sum()))
        v = res[k][np.isfinite(res[k])]
        c = got[k].reshape((-1,) + got[k].shape[-2:]).sum(axis=0) if spec.ordinate is not None else got[k].sum(axis=0)[None, :]
        total, interior = int(c.sum()), c[..., 1:-1].sum(axis=0)
        outer = int(c[..., 0].sum() + c[..., -1].sum())
        print('%s %s: %d counted, %d interior cells of %d non-zero, %d in the outer bins' % (tag, k, total, int((interior > 0).sum()),
                                                                                           interior.size, outer))
        if not_empty and np.unique(v).size >= 3:
            assert int((interior > 0).sum()) >= 3, (tag, k, interior.tolist())
            assert outer < total, (tag, k, outer, total)


@pytest.mark.parametrize('cube', CUBES)
@pytest.mark.parametrize('name', NAMES)
def test_counts_of_the_rule(name, cube):
    op = op_for(name, cube)
    az, el = rays(name)
    plain, forms = plain_run(name, cube)
    for ordinate in ('heights', None):
        specs, fields = specs_for(name, cube, ordinate)
        assert len(fields) >= 9
        for i, spec in enumerate(specs):
            tag = '%s/cube %d/%s/%s' % (name, cube, ordinate, ('deciles', 'hand')[i])
            res = op.simulate_rays_histogram(az, el, spec, keep_gates=True)
            got, res = counts_of(res), arrays(res)
            assert op._ctx.launch_forms() == forms, tag
            for k, v in plain.items():                       # the per-gate arrays are those of the call without the histogram
                assert same(res[k], v), (tag, 'per-gate', k)
            assert_counts(got, res, spec, tag, not_empty=i == 0)
            if ordinate == 'heights' and i == 0:
                # per ray, and without the gates
                per_ray = op.simulate_rays_histogram(az, el, spec, keep_gates=True, rays_per_block=1)
                assert_counts(counts_of(per_ray), arrays(per_ray), spec, tag + '/per ray', rpb=1, not_empty=False)
                for k in spec.fields:
                    assert np.array_equal(counts_of(per_ray)[k].sum(axis=0, keepdims=True), got[k]), (tag, k)
                only = op.simulate_rays_histogram(az, el, spec)
                for k in GATE_FIELDS + ['mask', 'mask_sum8', 'model_vars']:
                    assert k not in only, k
                assert all(same(counts_of(only)[k], got[k]) for k in spec.fields), tag
                assert all(same(np.asarray(only['histogram']['edges'][k]), spec.edges[k]) for k in spec.fields)
                assert same(np.asarray(only['histogram']['ordinate_edges']), spec.ordinate_edges)


def test_stencils_and_forms_are_left_alone():
    """Five sweeps of one geometry with the histogram and five of another without: the same stencil forms (full, recording,
    replay ...) and launch forms sweep by sweep, and every sweep's arrays those of the plain call."""
    name = 'c2_rsg'
    conf, luts, cubes, _, _ = case(name)
    spec = specs_for(name, 2)[0][0]
    seen = {}
    for with_hist in (False, True):
        op = operator(conf, luts)
        load(op, cubes[2])
        az, el = rays(name)
        st, forms, out = [], [], []
        for i in range(5):
            res = op.simulate_rays_histogram(az, el, spec, keep_gates=True) if with_hist else op.simulate_rays(az, el)
            out.append((arrays(res), counts_of(res) if with_hist else None))
            st.append(op.stencil_state()['form'])
            forms.append(op._ctx.launch_forms())
        seen[with_hist] = (st, forms, out)
        op.close()
    print('stencil forms without / with the histogram:', seen[False][0], seen[True][0])
    assert seen[False][0] == seen[True][0] and seen[True][0][-1] == 2
    assert seen[False][1] == seen[True][1]
    for i in range(5):
        for k, v in seen[False][2][i][0].items():
            assert same(seen[True][2][i][0][k], v), (i, k)
        assert_counts(seen[True][2][i][1], seen[True][2][i][0], spec, 'sweep %d' % i)
        assert all(same(seen[True][2][i][1][k], seen[True][2][0][1][k]) for k in spec.fields)


def captured(op, az, el, spec, **kw):
    """simulate_rays_histogram, and copies of the cpol_sweep_params / cpol_ray_tables_t it handed to Context.run_sweep"""
    from cosmo_pol_amd import _native as N
    ctx, seen = op._ctx, {}
    orig = ctx.run_sweep

    def spy(p, t, o):
        seen['p'], seen['t'] = N.SweepParams.from_buffer_copy(p), N.RayTables.from_buffer_copy(t)
        return orig(p, t, o)
    ctx.run_sweep = spy
    try:
        res = op.simulate_rays_histogram(az, el, spec, **kw)
    finally:
        del ctx.run_sweep
    return res, seen['p'], seen['t']


@pytest.mark.parametrize('name', ['c2_rsg', 'c5_2mom_dop2_sub'])
def test_output_modes(name):
    """Blocking host buffers, device pointers and page-locked buffers (waited for, and pinned=True + wait) carry the same counts."""
    import torch
    from cosmo_pol_amd import _native as N
    H = HG()
    op = op_for(name, 2)
    az, el = rays(name)
    spec = specs_for(name, 2)[0][0]
    locked, p, t = captured(op, az, el, spec, keep_gates=True)
    want, gates = counts_of(locked), arrays(locked)
    assert_counts(want, gates, spec, name + '/page-locked')
    lazy = op.simulate_rays_histogram(az, el, spec, pinned=True)
    op.wait()
    assert all(same(counts_of(lazy)[k], want[k]) for k in spec.fields)
    # blocking: pageable host buffers, the call returns when they are filled
    h, keep = N.Context.histogram_struct(spec)
    bufs = {k: np.full(want[k].shape, 77, dtype=np.uint64) for k in spec.fields}
    for k, a in bufs.items():
        h.counts[H.FIELDS.index(k)] = a.ctypes.data
    o = N.Outputs()
    o.histogram = C.pointer(h)
    zh = np.empty(gates['ZH'].shape, dtype=np.float32)
    o.ZH = zh.ctypes.data
    q = N.SweepParams.from_buffer_copy(p)
    q.outputs_on_device = 0
    op._ctx.run_sweep(q, t, o)
    assert all(same(bufs[k], want[k]) for k in spec.fields) and same(zh, gates['ZH'])
    # device pointers: written in place
    dev = {k: torch.full((want[k].size,), 77, dtype=torch.int64, device='cuda') for k in spec.fields}
    for k, a in dev.items():
        h.counts[H.FIELDS.index(k)] = a.data_ptr()
    q.outputs_on_device = 1
    o.ZH = None
    op._ctx.run_sweep(q, t, o)
    op.wait()
    assert all(same(dev[k].cpu().numpy().view(np.uint64).reshape(want[k].shape), want[k]) for k in spec.fields)
    # ... and through the operator: device_outputs['histogram'], a pass of two calls
    dev2 = {k: torch.full((want[k].size,), 77, dtype=torch.int64, device='cuda') for k in spec.fields}
    ptrs = {'histogram': {k: a.data_ptr() for k, a in dev2.items()}}
    op.simulate_rays_histogram(az, el, spec, phase=1, device_outputs=ptrs)
    op.wait()
    assert all((a == 77).all().item() for a in dev2.values())           # nothing is written before the finish
    op.simulate_rays_histogram(az, el, spec, phase=2, device_outputs=ptrs)
    op.wait()
    assert all(same(dev2[k].cpu().numpy().view(np.uint64).reshape(want[k].shape), 2 * want[k]) for k in spec.fields)
    del keep


def test_pass_over_calls_of_different_shapes():
    """A pass folds calls of different ray counts and geometries when there is one block; the sum does not depend on the cut."""
    H = HG()
    name = 'c3_melt_ice'
    op = op_for(name, 0)
    az, el = rays(name)
    spec = specs_for(name, 0)[0][0]
    whole = op.simulate_rays_histogram(az, el, spec, keep_gates=True)
    a = op.simulate_rays_histogram(az[:3], el[:3], spec, phase=1, keep_gates=True)
    assert 'histogram' not in a
    b = op.simulate_rays_histogram(az[3:], el[3:] + 1.0, spec, phase=0, keep_gates=True)
    c = op.simulate_rays_histogram(az[3:], el[3:], spec, phase=2, keep_gates=True)
    want = H.count(arrays(c), spec, into=H.count(arrays(b), spec, into=H.count(arrays(a), spec)))
    got = counts_of(c)
    assert all(same(got[k], want[k]) for k in spec.fields)
    extra = H.count(arrays(b), spec)
    assert all(np.array_equal(got[k] - extra[k], counts_of(whole)[k]) for k in spec.fields)
    with pytest.raises(ValueError, match='no pass open'):
        op.simulate_rays_histogram(az, el, spec, phase=0)


def test_ensemble():
    H = HG()
    name = 'c4_7x7'
    op, _, _ = E.ensemble_operator(name)
    az, el = rays(name)
    first = arrays(op.simulate_rays_ensemble(az, el))
    fields = [k for k in GATE_FIELDS if k in first]
    spec = H.Histogram({k: decile_edges(first[k], H.dtype_of(k)) for k in fields}, ordinate='heights',
                       ordinate_edges=decile_edges(first['heights'], np.float32))
    kept = op.simulate_rays_ensemble_histogram(az, el, spec, keep_gates=True)
    got, gates = counts_of(kept), arrays(kept)
    assert gates['ZH'].shape[0] == 3 and gates['heights'].shape == gates['ZH'].shape[1:]
    for k in fields:
        assert same(gates[k], first[k]), k
    assert_counts(got, gates, spec, 'ensemble', rpb=len(az))
    only = op.simulate_rays_ensemble_histogram(az, el, spec)
    assert 'ZH' not in only and all(same(counts_of(only)[k], got[k]) for k in fields)
    whole = counts_of(op.simulate_rays_ensemble_histogram(az, el, spec, per_member=False))
    for k in fields:
        assert got[k].shape[0] == 3 and whole[k].shape[0] == 1
        assert np.array_equal(got[k].sum(axis=0, keepdims=True), whole[k]), k
    for m in range(3):
        op.select_member(m)
        alone = counts_of(op.simulate_rays_histogram(az, el, spec))
        for k in fields:
            assert same(got[k][m:m + 1], alone[k]), (m, k)
    op.select_member(0)
    assert not np.array_equal(got['ZH'][0], got['ZH'][1])
    # the member list cut into chunks: the same counts
    op.sequence_memory_budget = 1
    cut = op.simulate_rays_ensemble_histogram(az, el, spec)
    cut_whole = op.simulate_rays_ensemble_histogram(az, el, spec, per_member=False)
    op.sequence_memory_budget = None
    for k in fields:
        assert same(counts_of(cut)[k], got[k]) and same(counts_of(cut_whole)[k], whole[k]), k
    with pytest.raises(ValueError, match='model_vars'):
        op.simulate_rays_ensemble_histogram(az, el, H.Histogram({'ZH': [1.0, 2.0]}, ('model', 'T'), [250.0, 270.0]))
    op.close()


def test_time_blend():
    import test_gpu_timed as T
    H = HG()
    name = 'c4_7x7'
    op, _, _ = T.series_operator(name)
    az, el = rays(name)
    plain = T.arrays(op.simulate_rays_at(az, el, 200.0))
    fields = [k for k in GATE_FIELDS if k in plain]
    spec = H.Histogram({k: decile_edges(plain[k], H.dtype_of(k)) for k in fields}, ordinate='dist',
                       ordinate_edges=decile_edges(plain['dist'], np.float32))
    res = op.simulate_rays_at_histogram(az, el, 200.0, spec, keep_gates=True)
    got, gates = counts_of(res), arrays(res)
    for k, v in plain.items():
        assert same(gates[k], v), k
    assert_counts(got, gates, spec, 'timed')
    only = op.simulate_rays_at_histogram(az, el, 200.0, spec)
    assert 'ZH' not in only and all(same(counts_of(only)[k], got[k]) for k in fields)
    op.close()


def test_scans():
    H = HG()
    name = 'c2_rsg'
    op = op_for(name, 0, lanes=2)
    az, _ = rays(name)
    spec = specs_for(name, 0)[0][0]
    elevations = [4.0, 5.0, 6.0]
    singles = [counts_of(op.simulate_rays_histogram(az, np.full(len(az), e), spec)) for e in elevations]
    volume = op.get_PPI_histogram(elevations, spec, azimuths=az)
    assert len(volume['sweeps']) == 3 and 'ZH' not in volume['sweeps'][0]
    per_sweep = op.get_PPI_histogram(elevations, spec, azimuths=az, per_sweep=True)
    assert len(per_sweep) == 3
    for k in spec.fields:
        assert np.array_equal(counts_of(volume)[k], singles[0][k] + singles[1][k] + singles[2][k]), k
        for i in range(3):
            assert same(counts_of(per_sweep[i])[k], singles[i][k]), (i, k)
    assert not same(singles[0]['ZH'], singles[2]['ZH'])
    kept = op.get_PPI_histogram(elevations, spec, azimuths=az, keep_gates=True)
    want = {}
    for sweep in kept['sweeps']:
        H.count(arrays(sweep), spec, into=want)
    assert all(same(counts_of(kept)[k], want[k]) for k in spec.fields)
    rhi = op.get_RHI_histogram([az[0], az[1]], spec, elevations=[3.0, 4.0, 5.0, 6.0], keep_gates=True)
    want = {}
    for sweep in rhi['sweeps']:
        H.count(arrays(sweep), spec, into=want)
    assert all(same(counts_of(rhi)[k], want[k]) for k in spec.fields)
    assert len(op.get_RHI_histogram([az[0], az[1]], spec, elevations=[3.0, 4.0], per_sweep=True)) == 2


def test_cfad_by_temperature():
    """An ordinate ('model', 'T') on an operator that integrates the model variables; refused where they are not produced."""
    H = HG()
    name = 'c3_melt_ice'
    op = op_for(name, 0, output_variables='all')
    az, el = rays(name)
    plain = op.simulate_rays(az, el)
    names = list(op._staged_vars)
    iT = names.index('T')
    T = np.array(plain['model_vars'][iT])
    zh = np.array(plain['ZH'])
    spec = H.Histogram({'ZH': decile_edges(zh, np.float32), 'ZDR': decile_edges(np.array(plain['ZDR']), np.float32)},
                       ordinate=('model', 'T'), ordinate_edges=decile_edges(T, np.float64))
    res = op.simulate_rays_histogram(az, el, spec, keep_gates=True)
    got, gates = counts_of(res), arrays(res)
    assert same(gates['model_vars'], np.array(plain['model_vars'])) and same(gates['ZH'], zh)
    per_gate = dict(gates, model_vars={n: gates['model_vars'][i] for i, n in enumerate(names)})
    assert_counts(got, per_gate, spec, 'cfad by T')
    # without the gates the library integrates the model variables for the histogram alone
    only = op.simulate_rays_histogram(az, el, spec)
    assert 'model_vars' not in only and 'ZH' not in only
    assert all(same(counts_of(only)[k], got[k]) for k in spec.fields)
    f = H.frequencies(got['ZH'][0])
    assert f.shape == got['ZH'].shape[1:] and np.nanmax(f) <= 1.0
    with pytest.raises(ValueError, match='model_vars'):
        op_for(name, 0).simulate_rays_histogram(az, el, spec)            # output_variables='only_radar'
    with pytest.raises(ValueError, match='QX'):
        op.simulate_rays_histogram(az, el, H.Histogram({'ZH': [1.0, 2.0]}, ('model', 'QX'), [0.0, 1.0]))


def test_refusals_leave_the_context_usable():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import superob as SO
    H = HG()
    name = 'c2_rsg'
    op = op_for(name, 2)
    az, el = rays(name)
    spec = specs_for(name, 2)[0][0]
    good, p, t = captured(op, az, el, spec)
    good = counts_of(good)
    q = N.SweepParams.from_buffer_copy(p)
    q.outputs_on_device = 0

    def call(change=None, params=q, entry='run_sweep', outputs=None):
        h, keep = N.Context.histogram_struct(spec)
        bufs = {k: np.full(good[k].shape, 77, dtype=np.uint64) for k in spec.fields}
        for k, a in bufs.items():
            h.counts[H.FIELDS.index(k)] = a.ctypes.data
        if change:
            change(h)
        o = N.Outputs()
        o.histogram = C.pointer(h)
        if outputs:
            outputs(o)
        if entry == 'run_columns':
            op._ctx.run_columns(params, N.Columns(), o)
        else:
            op._ctx.run_sweep(params, t, o)
        del keep
        return bufs
    with pytest.raises(ValueError, match='phase'):
        call(lambda h: setattr(h, 'phase', 4))
    with pytest.raises(ValueError, match='rays_per_block'):
        call(lambda h: setattr(h, 'rays_per_block', 3))
    with pytest.raises(ValueError, match='ordinate'):
        call(lambda h: setattr(h, 'ordinate', 7))
    with pytest.raises(ValueError, match='model'):           # 32 + v where the call makes no model_vars
        call(lambda h: setattr(h, 'ordinate', 32))
    nodop = N.SweepParams.from_buffer_copy(q)
    nodop.simulate_doppler = 0
    if 'RVEL' in spec.fields:
        with pytest.raises(ValueError, match='RVEL'):
            call(params=nodop)
    with pytest.raises(ValueError, match='RVEL'):            # as ordinate (16 + 9), whatever fields the case has
        call(lambda h: setattr(h, 'ordinate', 25), params=nodop)
    # not together with another product; not through cpol_run_columns
    so = N.Superob()
    so.ray_window, so.gate_window, so.min_valid_fraction = 3, 5, 0.5
    zh = np.zeros(SO.shape(len(az), len(op.constants.RANGE_RADAR), SO.Superob(3, 5, 0.5)), dtype=np.float32)
    so.ZH = zh.ctypes.data
    with pytest.raises(ValueError, match='cpol_histogram: not together'):
        call(outputs=lambda o: setattr(o, 'superob', C.pointer(so)))
    ms, sm = N.MemberStats(), N.SpectrumMoments()
    with pytest.raises(ValueError, match='cpol_histogram: not together'):
        call(outputs=lambda o: setattr(o, 'member_stats', C.pointer(ms)))
    with pytest.raises(ValueError, match='cpol_histogram: not together'):
        call(outputs=lambda o: setattr(o, 'spectrum_moments', C.pointer(sm)))
    with pytest.raises(ValueError, match='histogram'):
        call(entry='run_columns')
    # nothing was queued, the context is usable: a good call with unchanged counts
    bufs = call()
    assert all(same(bufs[k], good[k]) for k in spec.fields)
    # the operator's own refusals
    with pytest.raises(ValueError):
        op.simulate_rays_histogram(az, el, {'ZH': [1.0, 2.0]})
    with pytest.raises(ValueError):
        op.simulate_rays_histogram(az, el, spec, rays_per_block=3)
    op.distributed = True
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_histogram(az, el, spec)
        with pytest.raises(NotImplementedError):
            op.get_PPI_histogram([4.0], spec, azimuths=az)
    finally:
        op.distributed = False
    high = op.config
    low = op.config
    high['radar']['coords'] = [46.5, 7.5, 400000.]
    op.config = high
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_histogram(az, el, spec)
    finally:
        op.config = low
    assert all(same(counts_of(op.simulate_rays_histogram(az, el, spec))[k], good[k]) for k in spec.fields)
