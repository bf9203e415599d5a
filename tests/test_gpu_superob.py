"""Superobservations on the GPU (cpol_outputs.superob, k_superob): every window average and every count of a call against
superob.average of that call's own per-gate arrays, bit for bit -- the rule is order-exact, so there is no tolerance -- and
the per-gate arrays, the launch forms, the gate stencils and a replayed graph against the same call without the field.

Cases: the golden radials c2_rsg (single beam), c3_melt_ice, c4_7x7 (49 sub-beams), c5_2mom_dop2_sub (Doppler scheme 2), seven
rays at az + 0.5 k, each with its own cube and with the planted-bad-values cube (perturbed(cube, 202, plant=True))."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

NAMES = ['c2_rsg', 'c3_melt_ice', 'c4_7x7', 'c5_2mom_dop2_sub']
CUBES = [0, 2]                                              # the case's own cube, and the planted one
N_RAYS = 7                                                  # R = 3 leaves a one-ray last window
FRACTIONS = [1.0, 0.5, 0.3]
GATE_FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL']
CLASSES = ['all_valid', 'some_valid_enough', 'some_valid_too_few', 'none_valid', 'partial', 'zdr_count_differs']

_ops = {}


@functools.lru_cache(maxsize=None)
def rays(name, n=N_RAYS):
    _, _, _, az, el = case(name)
    return az[0] + 0.5 * np.arange(n), np.full(n, el[0])


def op_for(name, cube=0, **kw):
    """One operator per (case, cube) for the module (the integral tables are built once)."""
    key = (name, cube, tuple(sorted(kw.items())))
    if key not in _ops:
        conf, luts, cubes, _, _ = case(name)
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


def windows(name):
    n_gates = len(op_for(name).constants.RANGE_RADAR)
    return [(1, 1), (3, 5), (7, 1), (8, n_gates), (2, n_gates + 3), (3, 64), (1, 65)]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def assert_superob(w, want, tag, fields=GATE_FIELDS):
    """the window averages and counts of a result == the restatement's"""
    n = 0
    for k in fields:
        assert (k in w) == (k in want), (tag, k)
        if k not in want:
            continue
        bad = int((~((w[k] == want[k]) | (np.isnan(w[k]) & np.isnan(want[k])))).sum()) if w[k].shape == want[k].shape else -1
        assert same(w[k], want[k]), (tag, k, w[k].dtype, want[k].dtype, w[k].shape, want[k].shape, bad)
        assert same(w['count'][k], want['count'][k]), (tag, k, 'count')
        n += 1
    assert n >= 9, (tag, n)
    return n


def copy_result(res):
    out = {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}
    if 'superob' in res:
        out['superob'] = {k: np.array(v) for k, v in res['superob'].items() if k != 'count'}
        out['superob']['count'] = {k: np.array(v) for k, v in res['superob']['count'].items()}
    return out


def tally(per_gate, spec, rpb=0):
    """How many windows of a call fall into each class, from the restatement, and the share of windows alive in ZH."""
    from cosmo_pol_amd import superob as SO
    got = SO.average(per_gate, spec, rpb)
    every = SO.average({'ZH': np.zeros_like(per_gate['ZH'])}, spec, rpb)['count']['ZH'].astype(np.int64)     # N of every window
    n = got['count']['ZH'].astype(np.int64)
    need = np.maximum(1, np.ceil(spec.min_valid_fraction * every.astype(np.float64)).astype(np.int64))
    t = {'all_valid': int((n == every).sum()), 'some_valid_enough': int(((n < every) & (n >= need)).sum()),
         'some_valid_too_few': int(((n >= 1) & (n < need)).sum()), 'none_valid': int((n == 0).sum()),
         'partial': int((every < spec.rays * spec.gates).sum()),
         'zdr_count_differs': int((got['count']['ZDR'] != got['count']['ZH']).sum())}
    assert np.array_equal(~np.isnan(got['ZH']), n >= need)
    return t, int((~np.isnan(got['ZH'])).sum()), n.size


@functools.lru_cache(maxsize=None)
def bits_run(name, cube):
    """Every window and fraction on one (case, cube): the assertions of test 1; -> (class tallies, windows alive in ZH, windows)."""
    from cosmo_pol_amd import superob as SO
    op = op_for(name, cube)
    az, el = rays(name)
    plain = copy_result(op.simulate_rays(az, el))
    forms = op._ctx.launch_forms()
    total, alive, n_win = dict.fromkeys(CLASSES, 0), 0, 0
    for R, G in windows(name):
        for frac in FRACTIONS:
            spec = SO.Superob(R, G, frac)
            tag = '%s/cube %d/%dx%d/%.1f' % (name, cube, R, G, frac)
            res = copy_result(op.simulate_rays_superob(az, el, spec, keep_gates=True))
            assert op._ctx.launch_forms() == forms, tag
            # the per-gate arrays are those of the call without the field
            for k, v in plain.items():
                assert same(res[k], v), (tag, 'per-gate', k)
            w = res['superob']
            assert_superob(w, SO.average(res, spec), tag)
            assert w['ZH'].shape == SO.shape(len(az), res['ZH'].shape[1], spec)
            if (R, G, frac) == (1, 1, 1.0):
                for k in GATE_FIELDS:
                    if k != 'ZDR':                          # (ZDR is the ratio of the powers, whatever the per-gate ZDR holds)
                        assert same(w[k], res[k]), (tag, 'identity', k)
            for k in ('lats', 'lons', 'dist', 'heights'):
                assert w[k].shape == w['ZH'].shape and w[k].dtype == res[k].dtype, (tag, k)
            t, a, n = tally(res, spec)
            print('%s: %s alive %d of %d' % (tag, t, a, n))
            for k in CLASSES:
                total[k] += t[k]
            alive += a
            n_win += n
    return total, alive, n_win


@functools.lru_cache(maxsize=None)
def hook_run():
    """k_superob on explicit per-gate arrays (Context.superob_fields), for what no sweep produces: the sweeps censor ZH and ZV
    together, so ZDR's gate set never differs from ZH's there (measured: 0 of 22 959 windows of the eight cases).  Random fields
    with gaps of their own per field, infinities, signed zeros; among the windows the largest one (255 x 257 = 65535 gates).
    -> class tallies."""
    from cosmo_pol_amd import superob as SO
    ctx = op_for('c2_rsg')._ctx
    rng = np.random.default_rng(11)
    total = dict.fromkeys(CLASSES, 0)
    for (n_rows, n_gates, rpb), specs in [((12, 70, 0), [(1, 1, 1.0), (3, 5, 0.5), (5, 64, 0.3), (12, 70, 0.7), (1, 65, 0.3)]),
                                          ((12, 70, 4), [(3, 8, 0.5), (2, 7, 1.0)]),
                                          ((300, 300, 0), [(255, 257, 0.3), (7, 9, 0.5)])]:
        f = {}
        for k in GATE_FIELDS:
            if k == 'ZDR':
                continue
            x = (rng.standard_normal((n_rows, n_gates)) * 10 ** rng.uniform(-3, 6)).astype(np.float64 if k == 'RVEL' else np.float32)
            if k in ('ZH', 'ZV'):
                x = np.abs(x)
            x[rng.random(x.shape) < 0.3] = np.nan                                  # gaps of its own per field
            x[rng.random(x.shape) < 0.01] = np.inf
            x[rng.random(x.shape) < 0.01] = -0.0
            x[:, :n_gates // 7] = np.nan                                            # windows without a gate
            f[k] = x
        f['ZV'][2:5, -n_gates // 5:] = f['ZH'][2:5, -n_gates // 5:] = 1.0          # ... and whole ones
        for R, G, frac in specs:
            spec = SO.Superob(R, G, frac)
            tag = 'hook %dx%d/%d: %dx%d/%.1f' % (n_rows, n_gates, rpb, R, G, frac)
            got = ctx.superob_fields(f, spec, rpb)
            want = SO.average(f, spec, rpb)
            assert_superob(got, want, tag)
            assert got['ZH'].shape == SO.shape(n_rows, n_gates, spec, rpb), tag
            t, a, n = tally(f, spec, rpb)
            print('%s: %s alive %d of %d' % (tag, t, a, n))
            for k in CLASSES:
                total[k] += t[k]
    # a requested field without its input, and the struct's own refusals, leave the context usable
    with pytest.raises(ValueError, match='no input'):       # (the library's own refusal: ZDR needs ZV)
        ctx.superob_fields({'ZH': f['ZH']}, SO.Superob(2, 2), want=['ZH', 'ZDR'])
    with pytest.raises(ValueError, match='no input'):
        ctx.superob_fields({'ZH': f['ZH']}, SO.Superob(2, 2), want=['KDP'])
    with pytest.raises(ValueError, match='ray_window'):     # (... and cpol_superob's, through the hook)
        ctx.superob_fields({'ZH': f['ZH']}, types.SimpleNamespace(rays=256, gates=256, min_valid_fraction=0.5))
    again = ctx.superob_fields({'ZH': f['ZH']}, SO.Superob(7, 9, 0.5))
    assert same(again['ZH'], want['ZH']) and list(again['count']) == ['ZH']
    return total


def test_kernel_on_explicit_fields():
    total = hook_run()
    assert total['zdr_count_differs'] >= 1 and total['partial'] >= 1, total


@pytest.mark.parametrize('cube', CUBES)
@pytest.mark.parametrize('name', NAMES)
def test_bits_of_the_restatement(name, cube):
    total, alive, n_win = bits_run(name, cube)
    assert n_win > 0


def test_every_class_of_window_occurred():
    """The bit tests do not pass vacuously: over the module every class of window occurred -- in the sweeps, except a ZDR count
    that differs from ZH's, which only the kernel run on explicit fields can show (hook_run) -- and in every case (a golden radial
    with one cube, over its windows and fractions -- a single call such as 8 x n_gates at fraction 1.0 is ONE window, dead as
    soon as one gate is censored) at least a quarter of the windows are alive in ZH."""
    total = dict.fromkeys(CLASSES, 0)
    for name in NAMES:
        for cube in CUBES:
            t, alive, n_win = bits_run(name, cube)
            print(name, cube, t, alive, n_win)
            assert 4 * alive >= n_win, (name, cube, alive, n_win)
            for k in CLASSES:
                total[k] += t[k]
    sweeps = dict(total)
    hook = hook_run()
    print('sweeps:', sweeps, 'explicit fields:', hook)
    assert sweeps['zdr_count_differs'] == 0, sweeps         # (k_final censors ZH and ZV together: the figure the documents quote)
    for k in CLASSES:
        if k != 'zdr_count_differs':                        # (see hook_run: no sweep can produce it)
            assert sweeps[k] >= 1, (k, sweeps)
        assert sweeps[k] + hook[k] >= 1, (k, sweeps, hook)


@pytest.mark.parametrize('name', ['c2_rsg', 'c5_2mom_dop2_sub'])
def test_without_keep_gates(name):
    from cosmo_pol_amd import superob as SO
    op = op_for(name, 2)
    az, el = rays(name)
    spec = SO.Superob(3, 5, 0.3)
    both = copy_result(op.simulate_rays_superob(az, el, spec, keep_gates=True))
    only = copy_result(op.simulate_rays_superob(az, el, spec))
    for k in GATE_FIELDS + ['mask', 'mask_sum8', 'DSPECTRUM', 'model_vars']:
        assert k not in only, k
    assert_superob(only['superob'], both['superob'], name)
    for k in ('lats', 'lons', 'dist', 'heights'):
        assert same(only['superob'][k], both['superob'][k]), k
        assert same(only['superob'][k], SO.coordinates(both, spec)[k]), k


def test_blocks():
    from cosmo_pol_amd import superob as SO
    name = 'c4_7x7'
    op = op_for(name, 2)
    az, el = rays(name, 8)
    spec = SO.Superob(3, 4, 0.5)
    one = copy_result(op.simulate_rays_superob(az, el, spec, keep_gates=True, rays_per_block=4))
    w = one['superob']
    assert w['ZH'].shape[0] == 4                            # 3 + 1, 3 + 1 rays
    assert_superob(w, SO.average(one, spec, rays_per_block=4), 'blocks')
    for b in range(2):
        part = copy_result(op.simulate_rays_superob(az[4 * b:4 * b + 4], el[4 * b:4 * b + 4], spec))['superob']
        for k in GATE_FIELDS:
            assert same(w[k][2 * b:2 * b + 2], part[k]), (b, k)
            assert same(w['count'][k][2 * b:2 * b + 2], part['count'][k]), (b, k)
        for k in ('lats', 'lons', 'dist', 'heights'):
            assert same(w[k][2 * b:2 * b + 2], part[k]), (b, k)
    whole = copy_result(op.simulate_rays_superob(az, el, spec))['superob']
    assert whole['ZH'].shape[0] == 3 and not same(whole['ZH'][1], w['ZH'][1])        # rays 3-5 against ray 3 alone
    with pytest.raises(ValueError):
        op.simulate_rays_superob(az, el, spec, rays_per_block=3)


@pytest.mark.parametrize('form', ['shared', 'per_member'])
def test_ensemble(form):
    from cosmo_pol_amd import superob as SO
    name = 'c4_7x7'
    op, _, _ = E.ensemble_operator(name)
    az, el = rays(name)
    spec = SO.Superob(3, 5, 0.3)
    got = op.simulate_rays_ensemble(az, el, form=form, superob=spec)
    kept = op.simulate_rays_ensemble(az, el, form=form, superob=spec, keep_gates=True)
    assert 'ZH' not in got and kept['ZH'].shape[0] == 3
    assert_superob(kept['superob'], SO.average(kept, spec), 'ensemble/' + form)
    assert_superob(got['superob'], kept['superob'], 'ensemble/%s/no gates' % form)
    assert got['superob']['ZH'].shape == (3,) + SO.shape(len(az), kept['ZH'].shape[2], spec)
    assert got['superob']['lats'].shape == got['superob']['ZH'].shape[1:]
    for m in range(3):
        op.select_member(m)
        alone = op.simulate_rays_superob(az, el, spec)['superob']
        for k in GATE_FIELDS:
            assert same(got['superob'][k][m], alone[k]), (form, m, k)
            assert same(got['superob']['count'][k][m], alone['count'][k]), (form, m, k)
    op.select_member(0)
    assert int(np.isfinite(got['superob']['ZH']).sum()) > 0
    op.close()


def test_time_blend():
    import test_gpu_timed as T
    from cosmo_pol_amd import superob as SO
    name = 'c4_7x7'
    op, _, _ = T.series_operator(name)
    az, el = rays(name)
    spec = SO.Superob(3, 5, 0.3)
    plain = T.arrays(op.simulate_rays_at(az, el, 200.0))                             # weight 1 / 3: not dyadic
    res = copy_result(op.simulate_rays_at_superob(az, el, 200.0, spec, keep_gates=True))
    for k, v in plain.items():
        assert same(res[k], v), k
    assert_superob(res['superob'], SO.average(res, spec), 'timed')
    only = copy_result(op.simulate_rays_at_superob(az, el, 200.0, spec))
    assert 'ZH' not in only
    assert_superob(only['superob'], res['superob'], 'timed/no gates')
    assert int(np.isfinite(res['superob']['ZH']).sum()) > 0
    op.close()


def captured(op, az, el, **kw):
    """simulate_rays_superob, and copies of the cpol_sweep_params / cpol_ray_tables_t it handed to Context.run_sweep (the arrays they
    point into are kept by the operator's caches)."""
    from cosmo_pol_amd import _native as N
    ctx, seen = op._ctx, {}
    orig = ctx.run_sweep

    def spy(p, t, o):
        seen['p'], seen['t'] = N.SweepParams.from_buffer_copy(p), N.RayTables.from_buffer_copy(t)
        return orig(p, t, o)
    ctx.run_sweep = spy
    try:
        res = op.simulate_rays_superob(az, el, **kw)
    finally:
        del ctx.run_sweep
    return res, seen['p'], seen['t']


def native_superob(spec, n_cells, mode, fields, alloc):
    """(cpol_superob, {field: array-like}) with buffers from alloc(name, dtype, count)"""
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import superob as SO
    so = N.Superob()
    so.ray_window, so.gate_window, so.min_valid_fraction = spec.rays, spec.gates, spec.min_valid_fraction
    bufs = {}
    for k in fields:
        bufs[k], ptr = alloc(k, np.float64 if k == 'RVEL' else np.float32, n_cells)
        setattr(so, k, ptr)
    bufs['count'], so.count = alloc('count', np.uint16, len(SO.FIELDS) * n_cells)
    return so, bufs


@pytest.mark.parametrize('name', ['c2_rsg', 'c5_2mom_dop2_sub'])
def test_output_modes(name):
    """Blocking host buffers, device pointers and page-locked buffers (waited for, and pinned=True + wait) carry the same bits."""
    import torch
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import superob as SO
    op = op_for(name, 2)
    az, el = rays(name)
    spec = SO.Superob(3, 5, 0.3)
    locked, p, t = captured(op, az, el, superob=spec, keep_gates=True)
    locked = copy_result(locked)
    w = locked['superob']
    n_cells = w['ZH'].size
    lazy = op.simulate_rays_superob(az, el, spec, pinned=True)
    op.wait()
    assert_superob(copy_result(lazy)['superob'], w, 'pinned + wait')

    def check(bufs, get, tag):
        for k in GATE_FIELDS:
            assert same(get(bufs[k]).reshape(w[k].shape), w[k]), (tag, k)
            row = get(bufs['count']).reshape((len(SO.FIELDS),) + w[k].shape)[SO.FIELDS.index(k)]
            assert same(row, w['count'][k]), (tag, k, 'count')

    # blocking: pageable host buffers, the call returns when they are filled
    def host(k, dt, n):
        a = np.full(n, 77, dtype=dt)
        return a, a.ctypes.data
    so, bufs = native_superob(spec, n_cells, 0, GATE_FIELDS, host)
    o = N.Outputs()
    o.superob = C.pointer(so)
    zh = np.empty(locked['ZH'].shape, dtype=np.float32)
    o.ZH = zh.ctypes.data
    q = N.SweepParams.from_buffer_copy(p)
    q.outputs_on_device = 0
    op._ctx.run_sweep(q, t, o)
    check(bufs, lambda a: a, 'blocking')
    assert same(zh, locked['ZH'])

    # device pointers: written in place
    def dev(k, dt, n):
        a = torch.full((n,), 77, dtype={np.float32: torch.float32, np.float64: torch.float64, np.uint16: torch.int16}[dt],
                       device='cuda')
        return a, a.data_ptr()
    so, bufs = native_superob(spec, n_cells, 1, GATE_FIELDS, dev)
    o = N.Outputs()
    o.superob = C.pointer(so)
    q.outputs_on_device = 1
    op._ctx.run_sweep(q, t, o)
    op.wait()
    check(bufs, lambda a: a.cpu().numpy().view(np.uint16) if a.dtype == torch.int16 else a.cpu().numpy(), 'device')
    # ... and through the operator: device_outputs['superob']
    so2, bufs2 = native_superob(spec, n_cells, 1, ['ZH', 'ZDR'], dev)
    op.simulate_rays_superob(az, el, spec, device_outputs={'superob': {'ZH': so2.ZH, 'ZDR': so2.ZDR, 'count': so2.count}})
    op.wait()
    cnt = bufs2['count'].cpu().numpy().view(np.uint16).reshape((len(SO.FIELDS),) + w['ZH'].shape)
    for k in ('ZH', 'ZDR'):
        assert same(bufs2[k].cpu().numpy().reshape(w[k].shape), w[k]), k
        assert same(cnt[SO.FIELDS.index(k)], w['count'][k]), k
    assert (cnt[SO.FIELDS.index('KDP')] == 77).all()        # only the rows of requested fields are written


def test_stencils_and_graphs_are_left_alone(monkeypatch):
    from cosmo_pol_amd import superob as SO
    name = 'c2_rsg'
    conf, luts, cubes, _, _ = case(name)
    az, el = rays(name)
    spec = SO.Superob(3, 5, 0.3)
    op = operator(conf, luts)
    load(op, cubes[2])
    first, forms = None, []
    for i in range(5):
        res = copy_result(op.simulate_rays_superob(az, el, spec))
        forms.append(op.stencil_state()['form'])
        if first is None:
            first = res
        assert_superob(res['superob'], first['superob'], 'sweep %d' % i)
    print('stencil forms of five superobservation sweeps:', forms)
    assert forms[-1] == 2, forms
    op.close()
    # a graph-replaying context: device outputs, unchanged arguments
    import torch
    monkeypatch.setenv('CPOL_USE_GRAPH', '1')
    op = operator(conf, luts)
    load(op, cubes[2])
    n_gates = len(op.constants.RANGE_RADAR)
    shape = SO.shape(len(az), n_gates, spec)
    gate = {k: torch.empty((len(az), n_gates), dtype=torch.float32, device='cuda') for k in ('ZH', 'ZV', 'KDP')}
    win = {k: torch.empty(shape, dtype=torch.float32, device='cuda') for k in ('ZH', 'KDP')}
    win['count'] = torch.zeros((len(SO.FIELDS),) + shape, dtype=torch.int16, device='cuda')
    ptrs = {k: v.data_ptr() for k, v in gate.items()}
    replayed = 0
    for _ in range(3):
        op.simulate_rays(az, el, device_outputs=ptrs)
        op.wait()
    plain = {k: v.cpu().numpy() for k, v in gate.items()}
    assert op._ctx.launch_forms()['graph_replayed'] == 1
    for _ in range(2):
        op.simulate_rays_superob(az, el, spec, device_outputs=dict(ptrs, superob={k: v.data_ptr() for k, v in win.items()}))
        op.wait()
        replayed = op._ctx.launch_forms()['graph_replayed']
    assert replayed == 1, 'a superobservation call no longer replays the sweep\'s graph'
    for k, v in gate.items():
        assert same(v.cpu().numpy(), plain[k]), k
    for k in ('ZH', 'KDP'):
        assert same(win[k].cpu().numpy(), first['superob'][k]), k
        assert same(win['count'].cpu().numpy().view(np.uint16)[SO.FIELDS.index(k)], first['superob']['count'][k]), k
    op.close()


def test_refusals_leave_the_context_usable():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import superob as SO
    name = 'c2_rsg'
    op = op_for(name, 2)
    az, el = rays(name)
    spec = SO.Superob(3, 5, 0.3)
    good, p, t = captured(op, az, el, superob=spec)
    good = copy_result(good)
    n_cells = good['superob']['ZH'].size
    q = N.SweepParams.from_buffer_copy(p)
    q.outputs_on_device = 0

    def host(k, dt, n):
        a = np.full(n, 77, dtype=dt)
        return a, a.ctypes.data

    def call(change, fields=('ZH', 'RVEL'), params=q):
        so, bufs = native_superob(spec, n_cells, 0, fields, host)
        change(so)
        o = N.Outputs()
        o.superob = C.pointer(so)
        op._ctx.run_sweep(params, t, o)
        return bufs

    def setter(**kw):
        def change(so):
            for k, v in kw.items():
                setattr(so, k, v)
        return change
    bad = [setter(ray_window=0), setter(gate_window=0), setter(ray_window=-3), setter(ray_window=256, gate_window=256),
           setter(min_valid_fraction=0.0), setter(min_valid_fraction=1.5), setter(min_valid_fraction=float('nan')),
           setter(min_valid_fraction=-0.5), setter(rays_per_block=-1), setter(rays_per_block=3), setter(rays_per_block=14),
           setter(ZH=None, RVEL=None)]
    for change in bad:
        with pytest.raises(ValueError):
            call(change)
    # RVEL without Doppler
    nodop = N.SweepParams.from_buffer_copy(q)
    nodop.simulate_doppler = 0
    with pytest.raises(ValueError):
        call(setter(), params=nodop)
    call(setter(), fields=('ZH',), params=nodop)            # (fine without RVEL)
    # nothing was queued, the context is usable: a good call with unchanged bits
    bufs = call(setter())
    assert same(bufs['ZH'].reshape(good['superob']['ZH'].shape), good['superob']['ZH'])
    assert same(bufs['RVEL'].reshape(good['superob']['RVEL'].shape), good['superob']['RVEL'])
    assert_superob(copy_result(op.simulate_rays_superob(az, el, spec))['superob'], good['superob'], 'after the refusals')
    # cpol_run_columns does not take the field
    with pytest.raises(ValueError, match='superob'):
        so, _ = native_superob(spec, n_cells, 0, ('ZH',), host)
        o = N.Outputs()
        o.superob = C.pointer(so)
        op._ctx.run_columns(q, N.Columns(), o)
    # the operator's own refusals
    with pytest.raises(ValueError):
        op.simulate_rays_superob(az, el, (3, 5))
    op.distributed = True
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_superob(az, el, spec)
    finally:
        op.distributed = False
    high = op.config
    low = op.config
    high['radar']['coords'] = [46.5, 7.5, 400000.]
    op.config = high
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_superob(az, el, spec)
    finally:
        op.config = low
    assert_superob(copy_result(op.simulate_rays_superob(az, el, spec))['superob'], good['superob'], 'at the end')


def test_scans():
    from cosmo_pol_amd import superob as SO
    name = 'c2_rsg'
    op = op_for(name, 0, lanes=2)
    az, _ = rays(name)
    spec = SO.Superob(3, 5, 0.3)
    elevations = [4.0, 5.0]
    scans = op.get_PPI_superob(elevations, spec, azimuths=az)
    assert len(scans) == 2
    for e, res in zip(elevations, scans):
        assert 'ZH' not in res
        alone = copy_result(op.simulate_rays_superob(az, np.full(len(az), e), spec))['superob']
        assert_superob(res['superob'], alone, 'ppi %g' % e)
        for k in ('lats', 'lons', 'dist', 'heights'):
            assert same(np.array(res['superob'][k]), alone[k]), k
    assert not same(np.array(scans[0]['superob']['ZH']), np.array(scans[1]['superob']['ZH']))
    rhi = op.get_RHI_superob([az[0]], spec, elevations=[3.0, 4.0, 5.0, 6.0], keep_gates=True)
    assert len(rhi) == 1 and rhi[0]['superob']['ZH'].shape[0] == 2 and 'ZH' in rhi[0]
    assert_superob(rhi[0]['superob'], SO.average(copy_result(rhi[0]), spec), 'rhi')
