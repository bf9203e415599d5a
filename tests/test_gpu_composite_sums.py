"""The exact sums of the composites on the GPU, the kernels alone (k_comp_sum and k_comp_sum_finish behind k_comp and
k_comp_finish, through cpol_debug_read "composite_fields"): hand-built rows no sweep produces, `sum`, `sum_skipped` and every
other map against composite.compose / composite.finish of the same rows.  The sums are formed by integer atomics and rounded
once, so every comparison here is exact (NaNs positionally equal), and it is made for BOTH lane forms of k_comp_sum: the runs of
equal (cell, exponent bin) of a wavefront summed first (1) and every lane on its own (2); form 0, the one the sweeps use, is
one of the two.

An azimuth of 90 degrees has sine exactly 1, so x = dist exactly: with x edges 0, 1, 2 ... a gate at dist = j + 0.5 lies in cell j."""
import math

import numpy as np
import pytest

from test_composite_sums_cpu import CELLS, OVERFLOW_TABLE, WAVY_TABLE, same
from test_gpu_composite import GRIDS, context, geometry, stretch, _ops

pytestmark = pytest.mark.gpu

F32 = np.float32
GATES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
Z_EDGES = {0: None, 1: [0.0, 1500.0], 3: [0.0, 500.0, 2000.0, 4000.0]}
# the specials of the CPU test (the [1e30, 1, -1e30] cell among them), NaN and both infinities included
POOL = np.array(sum(CELLS, []) + [1e30, 1.0, -1e30, 7.25e-12, -6.5e17, 3e38, -3e38, 0.75, -1.5, 3.0, 3.0], dtype=F32)


def CP():
    from cosmo_pol_amd import composite
    return composite


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def compare(got, want, spec, tag):
    assert sorted(got['sum']) == sorted(spec.fields) == sorted(got['sum_skipped']), tag
    for k in spec.fields:
        same(got['sum'][k], want['sum'][k], (tag, k, 'sum'))
        same(got['sum_skipped'][k], want['sum_skipped'][k], (tag, k, 'sum_skipped'))
        same(got['count'][k], want['count'][k], (tag, k, 'count'))
        assert list(got['values'][k]) == spec.planes(k), (tag, k)
        for p in spec.planes(k):
            same(got['values'][k][p], want['values'][k][p], (tag, k, p))


def check(fields, dist, heights, az, spec, rpb=0, tag='', forms=(1, 2), gate_xy=None):
    want = CP().finish(CP().compose(spec, fields, dist, heights, az, rays_per_block=rpb, gate_xy=gate_xy))
    for form in forms:
        got = context().composite_fields(fields, dist, heights, az, spec, rpb, lane_form=form, gate_xy=gate_xy)
        compare(got, want, spec, (tag, 'form', form))
    return want


def values(rng, shape, share=0.5):
    """Runs of equal values (a ray's neighbours share the exponent bin) broken by the specials."""
    x = np.repeat(rng.choice(POOL, (shape[0], (shape[1] + 6) // 7)), 7, axis=1)[:, :shape[1]].astype(F32)
    where = rng.random(shape) < share
    x[where] = rng.choice(POOL, int(where.sum()))
    return x


def spec_of(ex, ey, n_z, **kw):
    products = ('max', 'sum') if n_z else ('max', 'lowest', 'sum')
    return CP().Composite(['ZH', 'KDP'], ex, ey, products=products, z_edges=Z_EDGES[n_z], weight={'KDP': WAVY_TABLE}, **kw)


@pytest.mark.parametrize('n_z', sorted(Z_EDGES))
@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_every_gate_count_ray_count_grid_layers_and_block_shape(grid, n_z):
    assert stretch() == 1024
    rng = np.random.default_rng(17 + n_z)
    ex, ey = GRIDS[grid]
    spec = spec_of(ex, ey, n_z)
    summed = 0
    for n_gates in GATES:
        for n_rays in (1, 3):
            az, dist, heights = geometry(rng, n_rays, n_gates, ex, ey)
            fields = {'ZH': values(rng, (n_rays, n_gates)), 'KDP': values(rng, (n_rays, n_gates))}
            for rpb in (0, 1):
                want = check(fields, dist, heights, az, spec, rpb, (grid, n_z, n_gates, n_rays, rpb))
                summed += int(want['count']['ZH'].sum()) - int(want['sum_skipped']['ZH'].sum())
    assert summed > 100                                   # (no case passes on empty maps)


def test_the_cells_of_the_cpu_test_and_a_row_of_one_cell_with_alternating_exponents():
    from test_composite_sums_cpu import cells_row
    c = CP()
    v, x, _, h = cells_row()
    spec = c.Composite('ZH', np.arange(len(CELLS) + 1.0), [-1.0, 1.0], products=('max', 'sum'))
    want = check({'ZH': v}, x.astype(F32), h, [90.0], spec, tag='cells', forms=(0, 1, 2))
    got = want['sum']['ZH'][0, 0]
    assert got[0] == 1.0 and got[3] == 0.0 and not np.signbit(got[3]) and got[4] == 7.0 and np.isnan(got[5]) and np.isnan(got[6])
    for j, cell in enumerate(CELLS):
        t = [float(F32(q)) for q in cell if math.isfinite(q)]
        if t:
            assert got[j] == math.fsum(t) + 0.0, j
    # 1100 gates in ONE cell: the exponent bin changes from gate to gate, then in runs of three, across wavefront and stretch edges
    n = 1100
    a = np.where(np.arange(n) % 2 == 0, F32(1.0), F32(2.0 ** 20)).astype(F32)
    a[300:600] = np.where((np.arange(300) // 3) % 2 == 0, F32(-3.0 * 2.0 ** -130), F32(1.5 * 2.0 ** 100))
    a[1000:] = np.resize(np.array([1e30, 1.0, -1e30, 2.0 ** -149], dtype=F32), n - 1000)
    dist = np.full((1, n), 0.5, dtype=F32)
    spec = c.Composite('ZH', [0.0, 1.0, 2.0], [-1.0, 1.0], products=('max', 'sum'))
    want = check({'ZH': a[None]}, dist, np.zeros((1, n), dtype=F32), [90.0], spec, tag='one cell', forms=(0, 1, 2))
    assert want['count']['ZH'][0, 0, 0] == n and want['sum']['ZH'][0, 0, 0] == math.fsum(float(t) for t in a) and np.isnan(want['sum']['ZH'][0, 0, 1])
    # ... and every member a block: three rows of that kind, three maps
    rows = np.stack([a, a[::-1], -a])
    want = check({'ZH': rows}, dist, np.zeros((1, n), dtype=F32), [90.0], spec, rpb=1, tag='one cell, three blocks')
    assert [float(t) for t in want['sum']['ZH'][:, 0, 0]] == [math.fsum(float(t) for t in r) for r in rows]


@pytest.mark.parametrize('points', [2, 1024])
def test_weight_tables_with_gates_on_their_breakpoints(points):
    c = CP()
    rng = np.random.default_rng(points)
    tv = np.cumsum(rng.uniform(0.01, 2.0, points)).astype(F32)
    tf = rng.normal(0.0, 50.0, points)                    # (not monotonic)
    spec = c.Composite(['ZH', 'ZDR'], np.arange(6.0), [-1.0, 1.0], products=('max', 'sum'), weight={'ZH': (tv, tf), 'ZDR': OVERFLOW_TABLE})
    n = 1500
    pool = np.concatenate([tv, np.nextafter(tv, F32(np.inf)), np.nextafter(tv, F32(-np.inf)), POOL, (tv[:-1] + tv[1:]) / F32(2)]).astype(F32)
    v = rng.choice(pool, (2, n)).astype(F32)
    v[0, :points] = tv                                    # every breakpoint itself
    w = rng.choice(np.array([0.5, 1.0, 1.2, 1.5, 1.75, 2.0, 9.0, np.nan, np.inf, -np.inf], dtype=F32), (2, n))
    dist = rng.uniform(-0.0, 5.5, (1, n)).astype(F32)
    want = check({'ZH': v, 'ZDR': w}, dist, np.zeros((1, n), dtype=F32), [90.0], spec, tag=points, forms=(0, 1, 2))
    assert want['sum_skipped']['ZDR'].sum() > 0 and want['sum_skipped']['ZH'].sum() == 0 and np.isfinite(want['sum']['ZH']).all()


def test_the_gate_plane():
    c = CP()
    rng = np.random.default_rng(23)
    n_rays, n = 3, 700
    x, y = rng.uniform(-0.5, 4.5, (n_rays, n)), rng.uniform(-0.5, 2.5, (n_rays, n))
    x[rng.random(x.shape) < 0.05] = np.nan
    x[1] = np.sort(x[1])                                  # (one ray walks through the cells in order: long runs)
    heights = rng.choice(np.array([0.0, 250.0, 1000.0, np.nan], dtype=F32), (n_rays, n))
    spec = c.Composite(['ZH', 'KDP'], np.arange(5.0), np.arange(3.0), products=('lowest', 'sum'), plane='geographic', weight={'KDP': WAVY_TABLE},
                       height_range=(0.0, 1000.0))
    fields = {'ZH': values(rng, (2 * n_rays, n)), 'KDP': values(rng, (2 * n_rays, n))}
    check(fields, None, heights, None, spec, tag='gate plane', gate_xy=(x, y))
    check(fields, None, heights, None, spec, rpb=n_rays, tag='gate plane, blocks per member', gate_xy=(x, y))


def test_a_pass_of_three_calls_one_of_which_hits_nothing():
    c = CP()
    rng = np.random.default_rng(29)
    ex, ey = GRIDS['3x2']
    spec = spec_of(ex, ey, 0)
    calls = []
    for n_rays, n_gates in ((2, 300), (1, 77), (4, 1300)):
        az, dist, heights = geometry(rng, n_rays, n_gates, ex, ey)
        calls.append(({'ZH': values(rng, (n_rays, n_gates)), 'KDP': values(rng, (n_rays, n_gates))}, dist, heights, az))
    calls[1] = (calls[1][0], np.full_like(calls[1][1], 1e6), calls[1][2], calls[1][3])        # every gate outside the grid
    state = None
    for f, dist, heights, az in calls:
        state = c.compose(spec, f, dist, heights, az, state=state)
    want = c.finish(state)
    for form in (1, 2):
        for i, (f, dist, heights, az) in enumerate(calls):
            got = context().composite_fields(f, dist, heights, az, spec, phase=(1, 0, 2)[i], lane_form=form)
            assert got is None or i == 2
        compare(got, want, spec, ('three calls', form))
    # the middle call alone: nothing counted, every sum NaN, nothing skipped
    f, dist, heights, az = calls[1]
    got = context().composite_fields(f, dist, heights, az, spec)
    assert np.isnan(got['sum']['ZH']).all() and not got['sum_skipped']['KDP'].any() and not got['count']['ZH'].any()


def test_the_existing_products_are_those_of_a_spec_without_sum():
    c = CP()
    rng = np.random.default_rng(31)
    ex, ey = GRIDS['3x2']
    az, dist, heights = geometry(rng, 3, 1500, ex, ey)
    fields = {'ZH': values(rng, (6, 1500)), 'KDP': values(rng, (6, 1500))}
    kw = dict(thresholds={'ZH': [-1.0, 0.75], 'KDP': [0.0]}, height_range=(0.0, 3000.0))
    for rpb in (0, 3):
        with_sum = context().composite_fields(fields, dist, heights, az, c.Composite(['ZH', 'KDP'], ex, ey, products=('max', 'lowest', 'echo_top', 'sum'), **kw), rpb)
        plain_spec = c.Composite(['ZH', 'KDP'], ex, ey, products=('max', 'lowest', 'echo_top'), **kw)
        plain = context().composite_fields(fields, dist, heights, az, plain_spec, rpb)
        assert sorted(plain) == ['count', 'values'] and sorted(with_sum) == ['count', 'sum', 'sum_skipped', 'values']
        for k in plain_spec.fields:
            same(with_sum['count'][k], plain['count'][k], k)
            for p in plain_spec.planes(k):
                same(with_sum['values'][k][p], plain['values'][k][p], (k, p))
    layered = dict(z_edges=Z_EDGES[3], column={'ZH': c.vil_table()}, gaps='hold')
    with_sum = context().composite_fields(fields, dist, heights, az, c.Composite(['ZH', 'KDP'], ex, ey, products=('max', 'column', 'sum'), **layered))
    plain = context().composite_fields(fields, dist, heights, az, c.Composite(['ZH', 'KDP'], ex, ey, products=('max', 'column'), **layered))
    assert sorted(plain) == ['column', 'column_layers', 'count', 'values'] and with_sum['sum']['KDP'].shape == plain['count']['KDP'].shape == (1, 3, 2, 3)
    same(with_sum['column']['ZH'], plain['column']['ZH'])
    same(with_sum['column_layers']['ZH'], plain['column_layers']['ZH'])
    same(with_sum['values']['KDP']['max'], plain['values']['KDP']['max'])


def test_refusals_leave_the_pass_and_the_context_usable():
    c = CP()
    rng = np.random.default_rng(37)
    ex, ey = GRIDS['3x2']
    spec = spec_of(ex, ey, 0)
    az, dist, heights = geometry(rng, 2, 400, ex, ey)
    fields = {'ZH': values(rng, (2, 400)), 'KDP': values(rng, (2, 400))}
    ctx = context()
    once = c.finish(c.compose(spec, fields, dist, heights, az))
    ctx.composite_fields(fields, dist, heights, az, spec, phase=1)          # a pass is open while the refusals come
    other = (np.array([1.0, 2.0, 3.0], dtype=F32), np.array([0.0, 1.0, 0.5]))

    def call(tamper, phase=2, spec=spec):
        return ctx.composite_fields(fields, dist, heights, az, spec, phase=phase, tamper=tamper)
    for word, tamper in (('SUM stands beside', lambda w: setattr(w.c, 'products', 256)), ('SUM with SOURCE', lambda w: setattr(w.c, 'products', 257 + 16)),
                         ('products must name MAX, LOWEST or ECHO_TOP and no other bit', lambda w: setattr(w.c, 'products', 257 + 128)),
                         ('not requested', lambda w: (w.n_weight.__setitem__(1, 3), w.weight_v.__setitem__(1, other[0].ctypes.data), w.weight_f.__setitem__(1, other[1].ctypes.data))),
                         ('2 ... 1024', lambda w: w.n_weight.__setitem__(3, 1)), ('2 ... 1024', lambda w: w.n_weight.__setitem__(3, 1025)),
                         ('NULL', lambda w: w.weight_f.__setitem__(3, None)), ('sum and sum_skipped', lambda w: w.sum.__setitem__(0, None)),
                         ('sum and sum_skipped', lambda w: w.sum_skipped.__setitem__(3, None)),
                         ('a weight table differs', lambda w: (w.n_weight.__setitem__(0, 3), w.weight_v.__setitem__(0, other[0].ctypes.data), w.weight_f.__setitem__(0, other[1].ctypes.data))),
                         ('a weight table differs', lambda w: w.n_weight.__setitem__(3, 0)),
                         ('differ from the open pass', lambda w: setattr(w.c, 'products', 259 - 2))):
        with pytest.raises(ValueError, match=word):
            call(tamper)
    bad = (np.array([1.0, np.nan], dtype=F32), np.array([0.0, 1.0]))
    for word, table in (('NaN or infinite', bad), ('NaN or infinite', (other[0], np.array([0.0, np.inf, 1.0]))),
                        ('not strictly ascending', (np.array([1.0, 1.0], dtype=F32), np.array([0.0, 1.0])))):
        with pytest.raises(ValueError, match=word):
            call(lambda w, t=table: (w.n_weight.__setitem__(0, len(t[0])), w.weight_v.__setitem__(0, t[0].ctypes.data), w.weight_f.__setitem__(0, t[1].ctypes.data)))
    # a spec without 'sum' does not continue the pass of one with it
    with pytest.raises(ValueError, match='differ from the open pass'):
        ctx.composite_fields(fields, dist, heights, az, c.Composite(['ZH', 'KDP'], ex, ey, products=('max', 'lowest')), phase=2)
    # nothing was queued and the pass is as it was: it finishes with one more call folded -- every integer sum doubles exactly
    twice = call(None)
    for k in spec.fields:
        same(twice['count'][k], 2 * once['count'][k], k)
        same(twice['sum_skipped'][k], 2 * once['sum_skipped'][k], k)
        same(twice['sum'][k], 2.0 * once['sum'][k], k)
    with pytest.raises(ValueError, match='no pass open'):
        call(None, phase=0)
    compare(call(None, phase=3), once, spec, 'after the refusals')
