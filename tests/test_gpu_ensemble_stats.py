"""Ensemble statistics on the GPU (cpol_outputs.member_stats, k_member_fold / k_member_finish): the running fold against
ensemble_stats (the NumPy statement of the rule), bit for bit -- the rule is order-exact, so there is no tolerance; NaNs compare
equal whatever their payload.  First the kernels on explicit members through the test hook (cpol_debug_read
"member_stats_fields": sizes at the wavefront and workgroup edges, passes cut into calls, every value class), then end to end:
simulate_rays_ensemble_stats against ensemble_stats.reduce(simulate_rays_ensemble(...)) on the small radial cases and the three
members of tests/test_gpu_ensemble.py, whose member 2 carries planted NaN / -9999 values."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_ensemble as E

pytestmark = pytest.mark.gpu

FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL']
GEOM = ['lats', 'lons', 'dist', 'heights']
N_CELLS = [1, 63, 64, 65, 255, 256, 257, 1031]
PASSES = [[1], [2], [3], [5], [64], [64, 1], [64, 64, 2], [1, 1, 1, 1, 1]]
CLASSES = ['random', 'decades', 'subnormal', 'inf', 'negzero']
NAMES = ['c2_rsg', 'c4_7x7']                                # single beam with Doppler; 49 sub-beams

_ops = {}


def ens_op(name, **kw):
    """One ensemble operator per (case, keywords) for the module (the integral tables are built once)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _ops:
        _ops[key] = E.ensemble_operator(name, **kw)[0]
    return _ops[key]


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def assert_stats(got, want, tag):
    """every array of a statistics result == the restatement's: the same entries, dtype, shape, bits"""
    n = 0
    for kind, w in want.items():
        if kind == 'n_members':
            assert got.get('n_members', w) == w, tag
            continue
        assert set(got[kind]) == set(w), (tag, kind, sorted(got[kind]), sorted(w))
        for k, v in w.items():
            g = np.asarray(got[kind][k])
            bad = int((~((g == v) | ((g != g) & (v != v)))).sum()) if g.shape == v.shape else -1
            assert same(g, v), (tag, kind, k, g.dtype, v.dtype, g.shape, v.shape, bad)
            n += 1
    return n


# ---------------------------------------------------------------- the kernels on explicit members (the hook)
def members_of(cls, M, n_cells, T, need, rng):
    """[M, n_cells] of one value class, 20 % NaN, cell 0 all NaN, cell 1 with exactly need - 1 and cell 2 with exactly need
    counting members (where the shape has them)."""
    x = rng.standard_normal((M, n_cells))
    if cls == 'decades':
        x = x * 10.0 ** rng.integers(-4, 5, x.shape)
    elif cls == 'subnormal':
        # float32 / float64 subnormals, some of them zero.  (float64: the device's own division gave 4 of about 160 000 such means
        # one unit of the subnormal grid off -- member_div in cpol_member_stats.inl rounds a subnormal quotient once)
        x = x * (1e-40 if T == np.float32 else 1e-310)
    elif cls == 'negzero':
        x = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), x.shape)
    x = x.astype(T)
    if cls == 'inf':
        x[rng.random(x.shape) < 0.1] = np.inf
        x[rng.random(x.shape) < 0.1] = -np.inf
    x[rng.random(x.shape) < 0.2] = np.nan
    x[:, 0] = np.nan
    for cell, n in ((1, need - 1), (2, need)):
        if cell < n_cells and n <= M:
            x[:, cell] = np.nan
            x[rng.permutation(M)[:n], cell] = T(1.5)
    return x


def thresholds_of(x, n_thr, rng):
    """n_thr thresholds, most of them values of members (the comparison is a strict >), +-0.0 among them"""
    pool = x[np.isfinite(x)]
    thr = [0.0, -0.0] + ([float(v) for v in rng.choice(pool, 6)] if pool.size else [1.0] * 6)
    return [thr[(i + 1) % 8] for i in range(n_thr)]


@pytest.mark.parametrize('n_cells', N_CELLS)
def test_hook_against_the_rule(n_cells):
    from cosmo_pol_amd import ensemble_stats as ES
    ctx = ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(1000 + n_cells)
    combos = [(names, n_thr) for names in (FIELDS, ['RVEL']) for n_thr in (0, 1, 8)]
    seen, i = set(), 0
    for cut in PASSES:
        for cls in CLASSES:
            names, n_thr = combos[i % len(combos)]
            need = (1, 2, 3)[i % 3]
            i += 1
            M = sum(cut)
            rows = {k: members_of(cls, M, n_cells, ES.dtype_of(k), need, rng) for k in names}
            exceed = {k: thresholds_of(rows[k], n_thr, rng) for k in names} if n_thr else None
            spec = ES.EnsembleStats(extremes=True, exceed=exceed, fields=names, min_members=need)
            want = ES.reduce(rows, spec)
            tag = '%d cells, %r, %s, %d field(s), %d thr, need %d' % (n_cells, cut, cls, len(names), n_thr, need)
            at, got = 0, None
            for j, n in enumerate(cut):
                phase = (1 if j == 0 else 0) | (2 if j == len(cut) - 1 else 0)
                got = ctx.member_stats_fields({k: v[at:at + n] for k, v in rows.items()}, spec, phase=phase)
                assert (got is None) == (j < len(cut) - 1)
                at += n
            assert assert_stats(got, want, tag) == len(names) * (5 + (n_thr > 0)), tag
            seen.add((len(names), n_thr))
            if n_cells > 2 and M >= need:
                c = want['count'][names[0]]
                assert c[0] == 0 and c[1] == need - 1 and c[2] == need, tag
                assert np.isnan(want['mean'][names[0]][:2]).all() and not np.isnan(want['mean'][names[0]][2]), tag
    assert len(seen) == 6


def test_hook_fold_only_then_finish_without_members():
    from cosmo_pol_amd import ensemble_stats as ES
    ctx = ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(7)
    rows = {k: members_of('decades', 4, 300, ES.dtype_of(k), 2, rng) for k in ('ZH', 'RVEL')}
    spec = ES.EnsembleStats(extremes=True, exceed={'ZH': [0.0, 1.0]}, fields=['ZH', 'RVEL'], min_members=2)
    want = ES.reduce(rows, spec)
    assert ctx.member_stats_fields(rows, spec, phase=1) is None
    got = ctx.member_stats_fields({}, spec, phase=2, n_cells=300, names=('ZH', 'RVEL'))
    assert_stats(got, want, 'fold, then finish without members')
    # a pass begun without members, folded, and finished; and a pass of no member at all
    assert ctx.member_stats_fields({}, spec, phase=1, n_cells=300, names=('ZH', 'RVEL')) is None
    assert ctx.member_stats_fields(rows, spec, phase=0) is None
    assert_stats(ctx.member_stats_fields({}, spec, phase=2, n_cells=300, names=('ZH', 'RVEL')), want, 'begin without members')
    empty = ctx.member_stats_fields({}, spec, phase=3, n_cells=300, names=('ZH', 'RVEL'))
    assert_stats(empty, ES.reduce({k: v[:0] for k, v in rows.items()}, spec), 'no member')
    assert not empty['count']['ZH'].any() and np.isnan(empty['max']['RVEL']).all()


class Hook(C.Structure):
    pass


def raw_hook(ctx, x, change, phase, n_thr=2, outputs=True):
    """cpol_debug_read "member_stats_fields" on a struct built here: ZH alone, x [n_members, n_cells] float32, two thresholds,
    host outputs; `change(hook)` spoils it.  -> (return code, outputs)"""
    from cosmo_pol_amd import _native as N
    if not hasattr(Hook, '_fields_'):
        Hook._fields_ = [('n_members', C.c_int32), ('n_cells', C.c_int64), ('inp', C.c_void_p * 10), ('ms', N.MemberStats)]
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = Hook()
    h.n_members, h.n_cells = x.shape
    h.inp[0] = x.ctypes.data
    thr = np.array([1.0, 1.5], dtype=np.float64)
    h.ms.phase, h.ms.min_members, h.ms.fields = phase, 1, 1
    h.ms.n_thresholds[0], h.ms.thresholds[0] = n_thr, thr.ctypes.data
    out = {k: np.full(x.shape[1], 77, np.float32) for k in ('mean', 'spread', 'min', 'max')}
    out['count'] = np.full((10, x.shape[1]), 77, np.uint16)
    out['exceed'] = np.full((2, x.shape[1]), 77, np.uint16)
    if outputs:
        for k in ('mean', 'spread', 'min', 'max', 'exceed'):
            getattr(h.ms, k)[0] = out[k].ctypes.data
        h.ms.count = out['count'].ctypes.data
    keep = [thr]
    change(h, keep)
    rc = int(ctx.lib.cpol_debug_read(ctx.h, b'member_stats_fields', C.byref(h), C.sizeof(h)))
    return rc, out


def test_hook_refusals_leave_the_open_pass_alone():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import ensemble_stats as ES
    ctx = ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(3)
    x = members_of('random', 5, 257, np.float32, 1, rng)
    spec = ES.EnsembleStats(extremes=True, exceed={'ZH': [1.0, 1.5]}, fields=['ZH'])
    want = ES.reduce({'ZH': x}, spec)
    nan_thr = np.array([1.0, np.nan])
    other_thr = np.array([1.0, 1.25])

    def s(**kw):
        def change(h, keep):
            for k, v in kw.items():
                if k == 'n_thr':
                    h.ms.n_thresholds[0] = v
                elif k == 'thr':
                    keep.append(v)
                    h.ms.thresholds[0] = None if v is None else v.ctypes.data
                elif k == 'n_thr_other':
                    h.ms.n_thresholds[4] = v                # (a field that is not folded: the range is checked all the same)
                else:
                    setattr(h.ms, k, v)
        return change
    ok = s()
    few, more = x[3:], np.zeros((65533, 257), np.float32)
    # (what is wrong, the phase of the refused call, its members)
    bad = [(s(phase=4), 0, few), (s(phase=-1), 0, few), (s(phase=7), 0, few), (s(min_members=0), 0, few), (s(min_members=0), 1, few),
           (s(min_members=-2), 3, few), (s(fields=0), 0, few), (s(fields=0), 1, few), (s(fields=1 | 1 << 10), 1, few),
           (s(fields=1 << 31), 3, few), (s(n_thr=9), 1, few), (s(n_thr=-1), 0, few), (s(n_thr_other=9), 1, few),
           (s(thr=None), 1, few), (s(thr=nan_thr), 1, few), (s(thr=nan_thr), 0, few),
           # a fold that differs from the open pass: n_cells, fields, thresholds (their number, their values), min_members
           (ok, 0, x[3:, :256]), (s(fields=3), 0, few), (s(n_thr=1), 0, few), (s(thr=other_thr), 2, few), (s(min_members=2), 2, few),
           # more than 65535 members in the pass (3 are folded), and in one call that begins a pass
           (ok, 0, more), (ok, 1, np.zeros((65536, 1), np.float32))]
    for i, (change, phase, rows) in enumerate(bad):
        rc, _ = raw_hook(ctx, x[:3], ok, 1)
        assert rc == 0
        rc, out = raw_hook(ctx, rows, change, phase)
        assert rc == N.ERR_ARG, (i, phase, rc)
        assert (out['mean'] == 77).all() and (out['count'] == 77).all()
        rc, out = raw_hook(ctx, few, ok, 2)
        assert rc == 0
        got = {k: {'ZH': out[k]} for k in ('mean', 'spread', 'min', 'max', 'exceed')}
        got['count'] = {'ZH': out['count'][0]}
        assert_stats(got, want, 'after refusal %d' % i)
        assert (out['count'][1:] == 77).all()               # (host outputs: the rows of fields not folded are not written)
    # a finishing call without an output pointer: refused, the pass stays open and finishes
    assert raw_hook(ctx, x[:3], ok, 1)[0] == 0
    assert raw_hook(ctx, few, ok, 2, outputs=False)[0] == N.ERR_ARG
    rc, out = raw_hook(ctx, few, ok, 2)
    assert rc == 0 and same(out['mean'], want['mean']['ZH']) and same(out['exceed'], want['exceed']['ZH'])
    # no pass is open now: a fold and a finish without the begin bit are refused, a folded field needs its input
    assert raw_hook(ctx, few, ok, 0)[0] == N.ERR_ARG and raw_hook(ctx, few, ok, 2)[0] == N.ERR_ARG
    with pytest.raises(ValueError, match='no pass is open'):
        ctx.member_stats_fields({'ZH': x}, spec, phase=2)
    with pytest.raises(ValueError, match='no input'):
        ctx.member_stats_fields({'ZH': x}, spec, phase=3, names=('ZH', 'KDP'))
    with pytest.raises(ValueError):
        ctx.member_stats_fields({}, spec, phase=3, n_cells=0, names=('ZH',))
    assert_stats(ctx.member_stats_fields({'ZH': x}, spec), want, 'at the end')


# ---------------------------------------------------------------- end to end
def stats_spec(**kw):
    from cosmo_pol_amd import ensemble_stats as ES
    return ES.EnsembleStats(extremes=True, exceed={'ZH': [ES.dbz(0.0), ES.dbz(20.0)], 'KDP': [0.0]}, min_members=2, **kw)


def reference(op, az, el, spec, members=None, form='shared'):
    """(ensemble_stats.reduce of the members' own per-gate arrays, those arrays)"""
    from cosmo_pol_amd import ensemble_stats as ES
    full = op.simulate_rays_ensemble(az, el, members=members, form=form)
    full = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in full.items()}
    return ES.reduce(full, spec), full


def copy_stats(s):
    return {kind: (v if kind == 'n_members' else {k: np.array(a) for k, a in v.items()}) for kind, v in s.items()}


@pytest.mark.parametrize('name', NAMES)
def test_forms_chunks_and_member_order(name):
    op = ens_op(name)
    _, _, _, az, el = E.case(name)
    spec = stats_spec()
    want, full = reference(op, az, el, spec)
    assert ('RVEL' in want['mean']) == ('RVEL' in full) and len(want['mean']) >= 9
    assert name != 'c2_rsg' or 'RVEL' in want['mean']        # (the single-beam case runs a Doppler scheme)
    c = want['count']['ZH']
    assert ((c > 0) & (c < 3)).any() and (c == 3).any(), 'member 2\'s planted values do not lower a count'
    assert want['exceed']['ZH'].any() and want['exceed']['ZH'].shape == (2,) + full['ZH'].shape[1:]
    for form in ('shared', 'per_member', None):
        got = op.simulate_rays_ensemble_stats(az, el, spec, form=form)
        assert 'ZH' not in got and 'mask' not in got and got['stats']['n_members'] == 3
        assert assert_stats(got['stats'], want, '%s/%s' % (name, form)) >= 9 * 5 + 2
        for k in GEOM:
            assert same(got[k], full[k]), (form, k)
    forms_shared = None
    try:
        op.sequence_memory_budget = 1                       # no member fits: a chunk each
        got = op.simulate_rays_ensemble_stats(az, el, spec, form='shared')
        assert_stats(got['stats'], want, name + '/one member per chunk')
        forms_shared = op._ctx.launch_forms()
    finally:
        op.sequence_memory_budget = None
    assert forms_shared['interp_classify'] == 0
    # the order of the members matters to the bits
    want20, full20 = reference(op, az, el, spec, members=[2, 0])
    for form in ('shared', 'per_member'):
        got = op.simulate_rays_ensemble_stats(az, el, spec, members=[2, 0], form=form)
        assert got['stats']['n_members'] == 2
        assert_stats(got['stats'], want20, '%s/%s/[2, 0]' % (name, form))
    want02 = reference(op, az, el, spec, members=[0, 2])[0]
    assert same(want02['count']['ZH'], want20['count']['ZH']) and same(want02['max']['ZH'], want20['max']['ZH'])
    # fewer outputs: only what the specification asks for arrives
    from cosmo_pol_amd import ensemble_stats as ES
    lean = ES.EnsembleStats(spread=False, fields=['ZH', 'KDP'], exceed={'KDP': [0.0]})
    got = op.simulate_rays_ensemble_stats(az, el, lean, form='per_member')['stats']
    assert set(got) == {'mean', 'count', 'exceed', 'n_members'} and set(got['mean']) == {'ZH', 'KDP'}
    assert_stats(got, ES.reduce(full, lean), name + '/lean')


@pytest.mark.parametrize('name', NAMES)
def test_output_modes(name):
    """Blocking host buffers, page-locked buffers on another lane (pinned=True + wait) and device pointers carry the same bits."""
    import torch
    from cosmo_pol_amd import ensemble_stats as ES
    op = ens_op(name)
    _, _, _, az, el = E.case(name)
    spec = stats_spec()
    want, full = reference(op, az, el, spec)
    shape = full['ZH'].shape[1:]
    for form in ('shared', 'per_member'):
        got = op.simulate_rays_ensemble_stats(az, el, spec, form=form, lane=1, pinned=True)
        op.wait(1)
        assert_stats(got['stats'], want, '%s/%s/pinned on lane 1' % (name, form))
        names = list(want['mean'])
        dev = {kind: {k: torch.full(shape, 7, dtype=torch.float64 if k == 'RVEL' else torch.float32, device='cuda') for k in names}
               for kind in ('mean', 'spread', 'min', 'max')}
        dev['exceed'] = {k: torch.full((len(spec.exceed[k]),) + shape, 7, dtype=torch.int16, device='cuda') for k in spec.exceed}
        dev['count'] = torch.full((10,) + shape, 7, dtype=torch.int16, device='cuda')
        ptrs = {kind: (v.data_ptr() if kind == 'count' else {k: a.data_ptr() for k, a in v.items()}) for kind, v in dev.items()}
        res = op.simulate_rays_ensemble_stats(az, el, spec, form=form, lane=1, device_outputs={'stats': ptrs})
        op.wait(1)
        assert 'ZH' not in res
        cnt = dev.pop('count').cpu().numpy().view(np.uint16)
        got = {kind: {k: (a.cpu().numpy().view(np.uint16) if kind == 'exceed' else a.cpu().numpy()) for k, a in v.items()}
               for kind, v in dev.items()}
        got['count'] = {k: cnt[FIELDS.index(k)] for k in names}
        assert_stats(got, want, '%s/%s/device outputs' % (name, form))
        if 'RVEL' not in names:                             # (device outputs: the row of a field that is not folded stays the caller's)
            assert (cnt[FIELDS.index('RVEL')] == 7).all()
    with pytest.raises(ValueError):
        op.simulate_rays_ensemble(az, el, device_outputs={'stats': {}})


@pytest.mark.parametrize('name', NAMES)
def test_keep_members_and_the_calls_around(name):
    op = ens_op(name)
    _, _, _, az, el = E.case(name)
    spec = stats_spec()
    want, full = reference(op, az, el, spec)
    forms_ens = op._ctx.launch_forms()
    for _ in range(3):                                      # (three times: a single-beam sweep replays its gate stencil from the third)
        one = {k: np.array(v) for k, v in op.simulate_rays(az, el).items() if isinstance(v, np.ndarray)}
    forms_one = op._ctx.launch_forms()
    for form in ('shared', 'per_member'):
        kept = op.simulate_rays_ensemble_stats(az, el, spec, keep_members=True, form=form)
        assert_stats(kept['stats'], want, '%s/%s/keep_members' % (name, form))
        n = 0
        for k, v in full.items():
            if isinstance(v, np.ndarray):
                assert same(kept[k], v), (form, k)
                n += 1
        assert n >= 14 and set(kept) == set(full) | {'stats'}
        # an ordinary ensemble call, and a simulate_rays on the same lane directly afterwards: unchanged bits and launch forms
        op.simulate_rays_ensemble_stats(az, el, spec, form=form)
        again = op.simulate_rays_ensemble(az, el, form='shared')
        assert op._ctx.launch_forms() == forms_ens, form
        for k, v in full.items():
            if isinstance(v, np.ndarray):
                assert same(again[k], v), (form, 'ensemble afterwards', k)
        op.simulate_rays_ensemble_stats(az, el, spec, form=form)
        after = op.simulate_rays(az, el)
        assert op._ctx.launch_forms() == forms_one, form
        for k, v in one.items():
            assert same(after[k], v), (form, 'simulate_rays afterwards', k)


def test_ppi_over_two_lanes():
    name = 'c2_rsg'
    op = ens_op(name, lanes=2)
    _, _, _, az, el = E.case(name)
    spec = stats_spec()
    azimuths = az[0] + 0.5 * np.arange(3)
    elevations = [el[0], el[0] + 0.7, el[0] + 1.9]
    scans = op.get_PPI_ensemble_stats(elevations, spec, azimuths=azimuths, members=[1, 2, 0])
    assert len(scans) == 3
    for e, res in zip(elevations, scans):
        want, full = reference(op, azimuths, np.full(3, e), spec, members=[1, 2, 0])
        assert res['stats']['n_members'] == 3 and res['stats']['mean']['ZH'].shape == (3, full['ZH'].shape[2])
        assert_stats(res['stats'], want, 'PPI at %.1f' % e)
        assert same(res['heights'], full['heights'])
    rhi = op.get_RHI_ensemble_stats([az[0]], spec, elevations=elevations)
    assert len(rhi) == 1
    want = reference(op, np.full(3, az[0]), np.array(elevations), spec)[0]
    assert_stats(rhi[0]['stats'], want, 'RHI')


def test_refusals_of_the_sweeps_and_the_operator():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import ensemble_stats as ES
    from cosmo_pol_amd import superob as SO
    name = 'c2_rsg'
    op = ens_op(name)
    ctx = op._ctx
    _, _, _, az, el = E.case(name)
    spec = stats_spec()
    want, full = reference(op, az, el, spec)
    n_cells = full['ZH'][0].size
    seen = {}
    orig = ctx.run_sweep_members

    def spy(p, t, members, o):
        seen['p'], seen['t'] = N.SweepParams.from_buffer_copy(p), N.RayTables.from_buffer_copy(t)
        return orig(p, t, members, o)
    ctx.run_sweep_members = spy
    try:
        op.simulate_rays_ensemble_stats(az, el, spec, form='shared')
    finally:
        del ctx.run_sweep_members
    p, t = seen['p'], seen['t']
    p.outputs_on_device = 0
    mean = np.full(n_cells, 77, np.float32)

    def outputs(names=('ZH',), phase=3):
        ms, keep = N.Context.member_stats_struct(ES.EnsembleStats(), names, phase)
        ms.mean[0] = mean.ctypes.data
        o = N.Outputs()
        o.member_stats = C.pointer(ms)
        return o, (ms, keep)
    o, keep = outputs()
    ctx.run_sweep_members(p, t, [0, 1, 2], o)
    assert same(mean.reshape(want['mean']['ZH'].shape), ES.reduce(full, ES.EnsembleStats(fields=['ZH']))['mean']['ZH'])
    mean[:] = 77
    # superobservations in the same call
    so = N.Superob()
    so.ray_window, so.gate_window, so.min_valid_fraction = 1, 1, 0.5
    zh = np.zeros(n_cells * 3, np.float32)
    so.ZH = zh.ctypes.data
    o, keep = outputs()
    o.superob = C.pointer(so)
    with pytest.raises(ValueError, match='superob'):
        ctx.run_sweep_members(p, t, [0, 1, 2], o)
    # a time-blended call
    tb = N.RayTables.from_buffer_copy(t)
    lo, w = np.zeros(len(az), np.int32), np.zeros(len(az), np.float32)
    tb.time_blend, tb.ray_state, tb.ray_weight = 1, lo.ctypes.data, w.ctypes.data
    o, keep = outputs()
    with pytest.raises(ValueError, match='time'):
        ctx.run_sweep_members(p, tb, [0, 1], o)
    # RVEL without Doppler; cpol_run_columns
    nodop = N.SweepParams.from_buffer_copy(p)
    nodop.simulate_doppler = 0
    o, keep = outputs(names=('ZH', 'RVEL'))
    with pytest.raises(ValueError, match='RVEL'):
        ctx.run_sweep_members(nodop, t, [0, 1, 2], o)
    o, keep = outputs()
    with pytest.raises(ValueError, match='member_stats'):
        ctx.run_columns(p, N.Columns(), o)
    # a fold-only sweep with no pass open
    o, keep = outputs(phase=0)
    with pytest.raises(ValueError, match='no pass is open'):
        ctx.run_sweep(p, t, o)
    assert (mean == 77).all()
    # the operator's own refusals
    with pytest.raises(ValueError):
        op.simulate_rays_ensemble_stats(az, el, (True, True))
    with pytest.raises(ValueError):
        op.simulate_rays_ensemble_stats(az, el, spec, members=[0, 0])
    # (a call takes ONE product, so statistics never meet superobservations: what an ensemble call refuses of
    # superobservations, and the calls the statistics do not share)
    with pytest.raises(ValueError, match='superobservations'):
        op._ensemble_rays(az, el, None, {'ZH': 1}, True, 0, 'per_member', False, SO.Windows(SO.Superob(1, 1)))
    with pytest.raises(ValueError, match='time-blended'):
        op._run_rays(az, el, op.config['radar']['coords'], full['ZH'].shape[2], 0.0, N.GEOM_GROUND_43,
                     timed=([0, 1], lo, w), product=ES.Fold(spec, False))
    with pytest.raises(ValueError, match='sub-beam'):
        op._run_rays(az, el, op.config['radar']['coords'], full['ZH'].shape[2], 0.0, N.GEOM_GROUND_43,
                     subbeams={}, product=ES.Fold(spec, False))
    if 'RVEL' not in full:
        with pytest.raises(ValueError, match='RVEL'):
            op.simulate_rays_ensemble_stats(az, el, ES.EnsembleStats(fields=['RVEL']))
    op.distributed = True
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_ensemble_stats(az, el, spec)
        with pytest.raises(NotImplementedError):
            op.get_PPI_ensemble_stats([1.0], spec, azimuths=az)
    finally:
        op.distributed = False
    high, low = op.config, op.config
    high['radar']['coords'] = [46.5, 7.5, 400000.]
    op.config = high
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_ensemble_stats(az, el, spec)
    finally:
        op.config = low
    # nothing was queued and no pass was left half open: a good call with unchanged bits
    assert_stats(op.simulate_rays_ensemble_stats(az, el, spec)['stats'], want, 'at the end')
