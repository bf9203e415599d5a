"""Where a call's output arrays are written (cosmo_pol_amd/csrc/cpol_place.h through run_sequence): the same call with blocking host
arrays, with device arrays, with one pinned slab whose arrays lie 4 bytes apart at most (the window form: one device image, one copy)
and with a pinned slab whose arrays lie too far apart for a window (buffers of the context, one copy per array).  Every array of
every form is compared bit for bit with the blocking-host form of the same call: that form is the reference among the four.

The sweep: the golden radial c2_rsg cut to 65 gates (a wavefront and one gate), 3 rays, one sub-beam, Doppler scheme 1 -- 195 float32
values are 780 bytes, so every float32 array moves the next address from 0 to 4 mod 8 and back, and the float64 arrays (RVEL, mask,
lats, lons) sit among them.  Alone, with superobservations (2 x 4 windows; ZH, RVEL and count), and as a two-member
cpol_run_sweep_members call with a beginning-and-finishing cpol_member_stats (the means of ZH and RVEL, count, one exceedance
threshold of ZH, the median of RVEL).  The rows of `count` that belong to fields nobody asked for are zeros in the window form (the
kernel writes them: the image is copied whole) and keep what the caller had there in every other form.

And the refusals that moved in front of the table upload: after each the table-upload entries of "host_times" are untouched and the
next good sweep carries the bits of the first."""
import copy
import ctypes as C

import numpy as np
import pytest

import test_gpu_ensemble as E

pytestmark = pytest.mark.gpu

N_RAYS, N_GATES = 3, 65
SENTINEL = 0x4D
F4, F8, I1, U2 = np.float32, np.float64, np.int8, np.uint16
POL = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V']
GAP = 1 << 16                       # between two arrays of the slab without a window: far more than a quarter of all arrays + 4096


def conf_65():
    conf, luts, cubes, az, el = E.case('c2_rsg')
    conf = copy.deepcopy(conf)
    conf['radar']['range'] = N_GATES * conf['radar']['radial_resolution']
    return conf, luts, cubes, az[0] + 0.5 * np.arange(N_RAYS), np.full(N_RAYS, el[0])


@pytest.fixture(scope='module')
def sweep_op():
    conf, luts, cubes, az, el = conf_65()
    op = E.operator(conf, luts)
    E.load(op, cubes[0])
    yield op, az, el
    op.close()


def spied(ctx, method, call):
    """call(), and copies of the cpol_sweep_params / cpol_ray_tables_t (and whatever else) it handed to ctx.<method>"""
    from cosmo_pol_amd import _native as N
    seen, orig = {}, getattr(ctx, method)

    def spy(p, t, *rest):
        seen['p'], seen['t'], seen['rest'] = N.SweepParams.from_buffer_copy(p), N.RayTables.from_buffer_copy(t), rest[:-1]
        return orig(p, t, *rest)
    setattr(ctx, method, spy)
    try:
        res = call()
    finally:
        delattr(ctx, method)
    return res, seen['p'], seen['t'], seen['rest']


def sweep_entries(n_rows, n_geo_rows):
    """[(name, dtype, count)] of a sweep's own arrays in slab order: float64 arrays among the float32 ones"""
    n, g = n_rows * N_GATES, n_geo_rows * N_GATES
    return [('ZH', F4, n), ('RVEL', F8, n), ('ZV', F4, n), ('mask', F8, n), ('ZDR', F4, n), ('lats', F8, g), ('KDP', F4, n),
            ('mask_sum8', I1, n), ('DELTA_HV', F4, n), ('lons', F8, g), ('PHIDP', F4, n), ('RHOHV', F4, n), ('dist', F4, g),
            ('ATT_H', F4, n), ('heights', F4, g), ('ATT_V', F4, n), ('sz_total', F4, 12 * n)]


def offsets(entries, start, gap_after=None):
    """every array at the next multiple of its item size, of 4 at least, from `start` on; GAP bytes behind entry `gap_after`"""
    at, out = start, {}
    for i, (name, dt, count) in enumerate(entries):
        a = max(4, np.dtype(dt).itemsize)
        at = (at + a - 1) // a * a
        out[name] = at
        at += count * np.dtype(dt).itemsize + (GAP if i == gap_after else 0)
    return out, at


def four_forms(ctx, entries, run):
    """run(mode, {name: address}) with the arrays of `entries` in each of the four forms -> {form: {name: array}}"""
    import torch
    got = {}
    for form, mode, start, gap_after in (('host', 0, 0, None), ('device', 1, 0, None), ('window', 2, 4, None), ('far', 2, 4, 1)):
        off, total = offsets(entries, start, gap_after)
        if form == 'device':
            slab = torch.full((total,), SENTINEL, dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()                            # (filled on torch's stream, written on the context's)
            base = slab.data_ptr()
        else:
            slab = ctx.host_alloc(total + 64) if mode == 2 else np.empty(total + 64, np.uint8)
            skip = -slab.ctypes.data % 64
            slab = slab[skip:skip + total]
            slab[:] = SENTINEL
            base = slab.ctypes.data
        assert base % 64 == 0
        if start:                                               # the lowest array float32 at 4 mod 8, a float64 array behind it
            (n0, d0, _), (n1, d1, _) = entries[0], entries[1]
            assert (d0, d1) == (F4, F8) and (base + off[n0]) % 8 == 4 and (base + off[n1]) % 8 == 0
            assert off[n1] == off[n0] + entries[0][2] * 4
        run(mode, {name: base + off[name] for name, _, _ in entries})
        ctx.synchronize()
        host = slab.cpu().numpy() if form == 'device' else slab
        got[form] = {name: host[off[name]:off[name] + count * np.dtype(dt).itemsize].view(dt).copy() for name, dt, count in entries}
    return got


def assert_forms_equal(got, entries, rows=None):
    """every array of every form == the blocking-host form's, bit for bit (`rows`: {name: (n_rows, rows compared)} of the count arrays)"""
    ref = got['host']
    for form in ('device', 'window', 'far'):
        for name, dt, count in entries:
            a, b = got[form][name], ref[name]
            if rows and name in rows:
                n, asked = rows[name]
                a, b = a.reshape(n, -1)[asked], b.reshape(n, -1)[asked]
            assert a.tobytes() == b.tobytes(), (form, name, int((a.view(np.uint8) != b.view(np.uint8)).sum()))
    for name, dt, count in entries:                             # (not vacuous: the reference was written)
        if not (rows and name in rows):
            assert ref[name].tobytes() != bytes([SENTINEL]) * ref[name].nbytes, name


def assert_other_rows(got, name, n_rows, asked):
    """the rows of a count array nobody asked for: zeros in the window form, the caller's bytes everywhere else"""
    rest = [r for r in range(n_rows) if r not in asked]
    for form in ('host', 'device', 'window', 'far'):
        r = got[form][name].reshape(n_rows, -1)[rest]
        want = 0 if form == 'window' else SENTINEL * 0x0101
        assert (r == want).all(), (form, name, np.unique(r))
    for form in got:
        assert not (got[form][name].reshape(n_rows, -1)[asked] == SENTINEL * 0x0101).all(), (form, name)


def sweep_outputs(addr):
    from cosmo_pol_amd import _native as N
    o = N.Outputs()
    for name in N.OUTPUT_FIELDS:
        if name in addr:
            setattr(o, name, addr[name])
    return o


def sweep_forms(sweep_op):
    """the sweep alone -> ({form: {name: array}}, entries)"""
    from cosmo_pol_amd import _native as N
    op, az, el = sweep_op
    ctx = op._ctx
    res, p, t, _ = spied(ctx, 'run_sweep', lambda: op.simulate_rays(az, el))
    assert (p.n_rays, p.n_gates, p.n_sub, p.simulate_doppler) == (N_RAYS, N_GATES, 1, 1)
    entries = sweep_entries(N_RAYS, N_RAYS)

    def run(mode, addr):
        q = N.SweepParams.from_buffer_copy(p)
        q.outputs_on_device = mode
        ctx.run_sweep(q, t, sweep_outputs(addr))
    return four_forms(ctx, entries, run), entries


def test_sweep(sweep_op):
    got, entries = sweep_forms(sweep_op)
    assert_forms_equal(got, entries)
    assert int(np.isfinite(got['host']['ZH']).sum()) > N_GATES and int(np.isfinite(got['host']['RVEL']).sum()) > N_GATES


def superob_forms(sweep_op):
    """the sweep with superobservations -> ({form: {name: array}}, entries, rows of count, rows asked for)"""
    from cosmo_pol_amd import _native as N
    op, az, el = sweep_op
    ctx = op._ctx
    _, p, t, _ = spied(ctx, 'run_sweep', lambda: op.simulate_rays(az, el))
    cells = -(-N_RAYS // 2) * -(-N_GATES // 4)                  # 2 x 4 windows: 2 x 17
    n_f = len(N.SUPEROB_FIELDS)
    asked = [N.SUPEROB_FIELDS.index('ZH'), N.SUPEROB_FIELDS.index('RVEL')]
    entries = sweep_entries(N_RAYS, N_RAYS)
    entries[3:3] = [('so.RVEL', F8, cells)]
    entries[7:7] = [('so.count', U2, n_f * cells)]
    entries[11:11] = [('so.ZH', F4, cells)]

    def run(mode, addr):
        q = N.SweepParams.from_buffer_copy(p)
        q.outputs_on_device = mode
        so = N.Superob()
        so.ray_window, so.gate_window, so.min_valid_fraction = 2, 4, 0.5
        so.ZH, so.RVEL, so.count = addr['so.ZH'], addr['so.RVEL'], addr['so.count']
        o = sweep_outputs(addr)
        o.superob = C.pointer(so)
        ctx.run_sweep(q, t, o)
    return four_forms(ctx, entries, run), entries, n_f, asked


def test_superob(sweep_op):
    got, entries, n_f, asked = superob_forms(sweep_op)
    assert_forms_equal(got, entries, rows={'so.count': (n_f, asked)})
    assert_other_rows(got, 'so.count', n_f, asked)
    assert int(np.isfinite(got['host']['so.ZH']).sum()) > 0


def member_stats_forms():
    """two members and their statistics -> ({form: {name: array}}, entries, rows of count, rows folded)"""
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import ensemble_stats as ES
    conf, luts, cubes, az, el = conf_65()
    op = E.operator(conf, luts)
    op.load_model_ensemble([c['data'] for c in cubes[:2]], cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    ctx = op._ctx
    _, p, t, (members,) = spied(ctx, 'run_sweep_members', lambda: op.simulate_rays_ensemble(az, el, members=[0, 1], form='shared'))
    # (n_rays: one member's rays; the call makes 2 * N_RAYS rows of them)
    assert (p.n_rays, p.n_gates, p.n_sub, p.simulate_doppler, list(members)) == (N_RAYS, N_GATES, 1, 1, [0, 1])
    cells = N_RAYS * N_GATES
    n_f = len(N.MEMBER_STATS_FIELDS)
    i_zh, i_rvel = N.MEMBER_STATS_FIELDS.index('ZH'), N.MEMBER_STATS_FIELDS.index('RVEL')
    spec = ES.EnsembleQuantiles({'RVEL': [0.5]}, spread=False, exceed={'ZH': [ES.dbz(0.0)]}, fields=['ZH', 'RVEL'])
    entries = sweep_entries(2 * N_RAYS, N_RAYS)
    entries[0:0] = [('ms.mean.ZH', F4, cells), ('ms.mean.RVEL', F8, cells)]
    entries[6:6] = [('ms.exceed.ZH', U2, cells)]
    entries[9:9] = [('ms.count', U2, n_f * cells)]
    entries[13:13] = [('ms.quantile.RVEL', F8, cells)]

    def run(mode, addr):
        q = N.SweepParams.from_buffer_copy(p)
        q.outputs_on_device = mode
        ms, keep = N.Context.member_stats_struct(spec, ('ZH', 'RVEL'), 3, capacity=2)
        ms.mean[i_zh], ms.mean[i_rvel] = addr['ms.mean.ZH'], addr['ms.mean.RVEL']
        ms.exceed[i_zh], ms.quantile[i_rvel], ms.count = addr['ms.exceed.ZH'], addr['ms.quantile.RVEL'], addr['ms.count']
        o = sweep_outputs(addr)
        o.member_stats = C.pointer(ms)
        ctx.run_sweep_members(q, t, members, o)
        del keep
    try:
        return four_forms(ctx, entries, run), entries, n_f, [i_zh, i_rvel]
    finally:
        op.close()


def test_member_stats():
    got, entries, n_f, (i_zh, i_rvel) = member_stats_forms()
    assert_forms_equal(got, entries, rows={'ms.count': (n_f, [i_zh, i_rvel])})
    assert_other_rows(got, 'ms.count', n_f, [i_zh, i_rvel])
    ref = got['host']
    assert int(np.isfinite(ref['ms.mean.ZH']).sum()) > 0 and int(np.isfinite(ref['ms.quantile.RVEL']).sum()) > 0
    assert int(ref['ms.count'].reshape(n_f, -1)[i_zh].max()) == 2


def test_refusals_queue_nothing(sweep_op):
    """The message texts are those of cosmo_pol_hip.hip at commit b5ad419 (lines 2572, 2592, 2605, 2613, 3005)."""
    from cosmo_pol_amd import _native as N
    op, az, el = sweep_op
    ctx = op._ctx
    _, p, t, _ = spied(ctx, 'run_sweep', lambda: op.simulate_rays(az, el))
    assert t.version != 0
    names = POL + ['RVEL', 'mask']

    def good():
        arrays = {k: np.full(N_RAYS * N_GATES, 77, F8 if k in ('RVEL', 'mask') else F4) for k in names}
        q = N.SweepParams.from_buffer_copy(p)
        q.outputs_on_device = 0
        ctx.run_sweep(q, t, sweep_outputs({k: a.ctypes.data for k, a in arrays.items()}))
        return arrays
    first = good()
    ctx.debug_read('host_times', (10,), np.float64)             # (reading resets the sums)
    sub = (np.zeros(64, np.int32), np.zeros(64, np.int32), np.full(64, 1.0 / 64))
    mask8 = np.zeros(N_RAYS * N_GATES, I1)

    def dop3(q, t2, o):
        q.simulate_doppler, q.n_vbins, t2.varray = 3, 64, None

    def broaden(q, t2, o):
        q.turbulence_correction = 1

    def dop2(q, t2, o):
        q.simulate_doppler = 2

    def sum8(q, t2, o):
        q.n_sub = 64
        t2.sub_h, t2.sub_v, t2.sub_w = sub[0].ctypes.data, sub[1].ctypes.data, sub[2].ctypes.data
        o.mask_sum8 = mask8.ctypes.data

    def wind(q, t2, o):
        q.var_u = -1
    cases = [(dop3, 'cpol_run_sweep: Doppler scheme 3 needs n_vbins in [2, 4097], tables->varray and var_rho'),
             (broaden, 'cpol_run_sweep: turbulence_correction / motion_correction need Doppler scheme 3'),
             (dop2, 'cpol_run_sweep: Doppler scheme 2 needs cpol_stage_doppler_weights'),
             (sum8, 'cpol_run_sweep: outputs->mask_sum8 needs 2 * n_sub <= 127 (one byte per gate)'),
             (wind, 'cpol_run_sweep: simulate_doppler needs var_u / var_v / var_w')]
    for i, (change, message) in enumerate(cases):
        q, t2 = N.SweepParams.from_buffer_copy(p), N.RayTables.from_buffer_copy(t)
        q.outputs_on_device = 0
        t2.version = t.version + 1000 + i                       # a new tag: the tables would have to be uploaded
        zh = np.full(N_RAYS * N_GATES, 77, F4)
        o = sweep_outputs({'ZH': zh.ctypes.data})
        change(q, t2, o)
        with pytest.raises(ValueError) as e:
            ctx.run_sweep(q, t2, o)
        assert str(e.value).endswith(message), (change.__name__, str(e.value))
        times = ctx.debug_read('host_times', (10,), np.float64)
        assert (times[6:10] == 0.0).all() and times[0] == 0.0, (change.__name__, times)
        assert (zh == 77).all()
        again = good()
        ctx.debug_read('host_times', (10,), np.float64)
        for k in names:
            assert again[k].tobytes() == first[k].tobytes(), (change.__name__, k)
    assert int(np.isfinite(first['ZH']).sum()) > N_GATES
