"""Height layers and the column of the gridded composites on the GPU, the kernels alone (k_comp<LAYERS>, k_comp_finish and
k_comp_column through cpol_debug_read "composite_fields"): hand-built rows no sweep produces, every plane, the count, the column
and its layer count against composite.compose / composite.finish / composite.column_of of the same rows.  The layered maps are
maxima and counts of integers, and the column is one thread's float64 sum over at most 64 layers in ascending order with
separately rounded operations, so every comparison here is bit for bit (NaNs positionally equal), for BOTH lane forms of k_comp.

S = the gates a workgroup owns.  An azimuth of 90 degrees has sine exactly 1, so x = dist exactly: with x edges 0, 1, 2 ... a
gate at dist = j + 0.5 lies in cell j."""
import numpy as np
import pytest

from test_gpu_composite import F32, GRIDS, _close_operators, context, same, stretch, values        # noqa: F401 (the fixture closes the operator)

pytestmark = pytest.mark.gpu

F64 = np.float64


def CP():
    from cosmo_pol_amd import composite
    return composite


def same_bits(got, want, tag):
    """Bit for bit for any dtype, NaNs positionally equal."""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != 'f':
        assert np.array_equal(got, want), (tag, got.ravel()[:16].tolist(), want.ravel()[:16].tolist())
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (tag, 'NaN positions', int(gn.sum()), int(wn.sum()))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, w = np.ascontiguousarray(got)[~gn].view(u), np.ascontiguousarray(want)[~wn].view(u)
    assert np.array_equal(g, w), (tag, int((g != w).sum()), got[~gn][g != w][:4].tolist(), want[~wn][g != w][:4].tolist())


def compare(got, want, spec, tag):
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for k in spec.fields:
        assert list(got['values'][k]) == ['max', 'height_of_max'], (tag, k)
        for p in ('max', 'height_of_max'):
            same(got['values'][k][p], want['values'][k][p], (tag, k, p))
        same(got['count'][k], want['count'][k], (tag, k, 'count'))
    for k in spec.column:
        same_bits(got['column'][k], want['column'][k], (tag, k, 'column'))
        same_bits(got['column_layers'][k], want['column_layers'][k], (tag, k, 'column_layers'))


def check(fields, dist, heights, az, spec, rpb=0, tag='', forms=(1, 2), gate_xy=None):
    c = CP()
    want = c.finish(c.compose(spec, fields, dist, heights, az, rays_per_block=rpb, gate_xy=gate_xy))
    for form in forms:
        got = context().composite_fields(fields, dist, heights, az, spec, rpb, lane_form=form, gate_xy=gate_xy)
        compare(got, want, spec, (tag, 'form', form))
    return want


def z_edges(n_z):
    """n_z layers whose edges are no round numbers in float32; the lowest edge below zero."""
    return -50.0 + 410.1 * np.arange(n_z + 1)


def height_pool(z):
    """Every edge, the value just under and just above each, both zeros, NaN and the infinities."""
    e = np.asarray(z, dtype=F32)
    return np.concatenate([e, np.nextafter(e, F32(-np.inf)), np.nextafter(e, F32(np.inf)), np.array([-0.0, 0.0, np.nan, np.inf, -np.inf], F32)])


TABLE2 = (np.array([-0.75, 1.5], F32), np.array([0.25, 7.0], F64))


def table1024():
    """1024 breakpoints over the value pool of `values` (-3 ... 3 in steps of 0.75 and the specials), uneven, with values that
    make every interpolation inexact."""
    tv = (-2.3 + 4.9 * (np.arange(1024) / 1023.0) ** 1.7).astype(F32)
    for on in (0.0, 0.75):                             # maxima ON a breakpoint
        tv[np.argmin(np.abs(tv - F32(on)))] = F32(on)
    assert np.all(tv[1:] > tv[:-1])
    return tv, 1e-3 * np.sqrt(np.arange(1024.0) + 0.3) * (1.0 + 0.1 * np.sin(np.arange(1024.0)))


def layered(grid, n_z, column=None, gaps='zero', fields=('ZH', 'ATT_V'), **kw):
    ex, ey = GRIDS[grid]
    if column is None:
        return CP().Composite(list(fields), ex, ey, z_edges=z_edges(n_z), **kw)
    return CP().Composite(list(fields), ex, ey, products=('max', 'column'), z_edges=z_edges(n_z), column=column, gaps=gaps, **kw)


def geometry(rng, n_rays, n_gates, grid, z):
    ex, ey = GRIDS[grid]
    az = rng.uniform(0.0, 360.0, n_rays)
    az[0] = 90.0
    reach = float(max(abs(ex[0]), abs(ex[-1]), abs(ey[0]), abs(ey[-1])))
    dist = rng.uniform(0.0, 1.2 * reach, (n_rays, n_gates)).astype(F32)
    dist[rng.random(dist.shape) < 0.03] = np.nan
    heights = rng.choice(height_pool(z), (n_rays, n_gates))
    return az, dist, heights


@pytest.mark.parametrize('n_z', [1, 2, 64])
@pytest.mark.parametrize('grid', ['1x1', '3x2'])
def test_every_stretch_length_ray_count_grid_layer_count_and_block_shape(grid, n_z):
    S = stretch()
    rng = np.random.default_rng(11 + n_z)
    spec = layered(grid, n_z, column={'ZH': TABLE2, 'ATT_V': table1024()}, gaps='hold')
    for n_gates in (1, 63, 64, 65, S - 1, S, S + 1):
        for n_rays in (1, 3):
            az, dist, heights = geometry(rng, n_rays, n_gates, grid, spec.z_edges)
            one = {k: values(rng, (n_rays, n_gates)) for k in spec.fields}
            check(one, dist, heights, az, spec, 0, '%s layers %d gates %d rays %d' % (grid, n_z, n_gates, n_rays))
            # two members over one geometry: one block of all rows, and n_rows / n_rays blocks
            two = {k: values(rng, (2 * n_rays, n_gates)) for k in spec.fields}
            for rpb in (0, n_rays):
                check(two, dist, heights, az, spec, rpb, '%s layers %d gates %d rays %d members 2 rpb %d' % (grid, n_z, n_gates, n_rays, rpb))


def test_rows_that_change_layer_every_gate_and_rows_of_one_layer():
    """The two extremes of the in-wavefront combine on (layer, cell): a steep ray, whose every gate lies in another layer, and a
    flat one, all of whose gates share a layer."""
    S = stretch()
    rng = np.random.default_rng(12)
    n = S + 65
    spec = layered('3x2', 64, column={'ZH': table1024()}, fields=('ZH',))
    z = spec.z_edges.astype(F64)
    mid = 0.5 * (z[1:] + z[:-1])
    dist = np.stack([np.full(n, 7.5, F32), rng.uniform(-5.0, 10.0, n).astype(F32), np.full(n, 20.0, F32)])
    az = np.array([90.0, 90.0, 90.0])
    heights = np.stack([mid[np.arange(n) % 64], np.full(n, mid[17]), mid[(np.arange(n) // 3) % 64]]).astype(F32)
    heights[0, 1::7] = z[(np.arange(n)[1::7] % 64) + 1].astype(F32)           # (on the edge above: the next layer, the last edge nowhere)
    v = values(rng, (3, n))
    want = check({'ZH': v}, dist, heights, az, spec, 0, 'steep and flat')
    cnt = want['count']['ZH'][0]
    assert (cnt.reshape(64, -1).sum(axis=1) > 0).all() and cnt[17].sum() > S // 2
    check({'ZH': np.concatenate([v, v[::-1]])}, dist, heights, az, spec, 3, 'steep and flat, two members')


def test_every_gate_in_one_layer_and_cell():
    """The contention extreme: 3 x (S + 1) gates, every one in the one (layer, cell), values and heights with many ties."""
    S = stretch()
    rng = np.random.default_rng(13)
    spec = layered('3x2', 64, column={'ZH': TABLE2}, fields=('ZH',))
    z = spec.z_edges
    n = S + 1
    dist = np.full((3, n), 7.5, F32)
    heights = rng.choice(np.array([z[40], np.nextafter(z[41], F32(0.0)), z[40] + F32(100.0)], F32), (3, n))
    v = rng.choice(np.array([-0.75, 0.0, 0.75, 0.75, 1.5, np.nan], F32), (3, n))
    want = check({'ZH': v}, dist, heights, np.full(3, 90.0), spec, 0, 'one layer and cell')
    cnt = want['count']['ZH'][0]
    assert cnt[40].sum() == int((v == v).sum()) == cnt.sum() and (cnt[40] > 0).sum() == 1


@pytest.mark.parametrize('n_z', [2, 64])
def test_the_gate_plane(n_z):
    """Per-gate coordinates in place of dist and the azimuths: the same layers behind them."""
    S = stretch()
    rng = np.random.default_rng(14)
    spec = layered('3x2', n_z, column={'ZH': TABLE2}, gaps='hold', fields=('ZH',), plane='geographic')
    for n_gates in (65, S + 1):
        x = rng.uniform(-45.0, 45.0, (3, n_gates))
        y = rng.uniform(-35.0, 35.0, (3, n_gates))
        x[rng.random(x.shape) < 0.05] = np.nan
        x[0, :4] = [-40.0, -5.0, 10.0, 40.0]
        heights = rng.choice(height_pool(spec.z_edges), (3, n_gates))
        v = values(rng, (6, n_gates))
        for rpb in (0, 3):
            check({'ZH': v}, None, heights, None, spec, rpb, 'gate plane layers %d gates %d rpb %d' % (n_z, n_gates, rpb), gate_xy=(x, y))


def test_a_pass_of_three_calls_and_one_that_hits_nothing():
    S = stretch()
    rng = np.random.default_rng(15)
    c, ctx = CP(), context()
    spec = layered('3x2', 64, column={'ZH': table1024(), 'ATT_V': TABLE2}, gaps='hold')
    for form in (1, 2):
        state, parts = None, []
        for i, (n_rays, n_gates) in enumerate(((2, 65), (1, S + 1), (3, 63), (2, 40))):
            az, dist, heights = geometry(rng, n_rays, n_gates, '3x2', spec.z_edges)
            if i == 3:
                heights[:] = spec.z_edges[-1]                  # (on the last edge: nowhere)
            f = {k: values(rng, (n_rays, n_gates)) for k in spec.fields}
            before = None if state is None else state['fields']['ZH']['count'].copy()
            state = c.compose(spec, f, dist, heights, az, state=state)
            if i == 3:
                assert np.array_equal(before, state['fields']['ZH']['count'])
            parts.append((f, dist, heights, az))
        for i, (f, dist, heights, az) in enumerate(parts):
            got = ctx.composite_fields(f, dist, heights, az, spec, phase=(1 if i == 0 else 2 if i == 3 else 0), lane_form=form)
            assert (got is None) == (i < 3)
        compare(got, c.finish(state), spec, ('pass of four calls', form))


VALUE_POOL = np.array([-3.0, -0.75, -0.7499999, 0.0, 0.3, 0.75, 1.4999999, 1.5, 1.5000001, 2.9, np.inf, -np.inf, 1e-45, -0.0], F32)


@pytest.mark.parametrize('gaps', ['zero', 'hold'])
@pytest.mark.parametrize('table', ['2 points', '1024 points'])
def test_the_column(table, gaps):
    """Cells with no layer, one layer, all 64 and random subsets of them; maxima below, on, between and above the breakpoints."""
    rng = np.random.default_rng(16)
    tab = TABLE2 if table == '2 points' else table1024()
    c = CP()
    spec = c.Composite('ZH', np.arange(9.0), [0.0, 1.0], products=('max', 'column'), z_edges=z_edges(64), column={'ZH': tab}, gaps=gaps)
    z = spec.z_edges.astype(F64)
    mid = (0.5 * (z[1:] + z[:-1])).astype(F32)
    pool = np.concatenate([VALUE_POOL, tab[0][[0, 1, -2, -1]], np.nextafter(tab[0][[0, -1]], F32(0.0)), np.nextafter(tab[0][[0, -1]], F32(9.0))])
    rows = []                                         # (cell, layer, value)
    rows += [(1, 23, v) for v in (0.3,)]                                          # cell 1: one layer; cell 0: none
    rows += [(2, l, rng.choice(pool)) for l in range(64)]                         # cell 2: all 64
    rows += [(3, l, rng.choice(pool)) for l in (0, 63)]                           # cell 3: the lowest and the highest, 62 held between
    rows += [(4, l, rng.choice(pool)) for l in range(64) if rng.random() < 0.3]
    rows += [(5, l, rng.choice(pool)) for l in range(64) if rng.random() < 0.7 for _ in range(3)]
    rows += [(6, l, F32(-3.0)) for l in (5, 9)]                                   # cell 6: below the table alone
    cell, layer, v = (np.array(a) for a in zip(*rows))
    order = rng.permutation(len(rows))
    dist = (cell[order] + 0.5).astype(F32)[None, :]
    want = check({'ZH': v[order].astype(F32)[None, :]}, dist, mid[layer[order]][None, :], [90.0], spec, 0, (table, gaps))
    col, lay = want['column']['ZH'][0, 0], want['column_layers']['ZH'][0, 0]
    assert np.isnan(col[0]) and lay[0] == 0 and lay[1] == 1 and lay[2] == 64 and lay[3] == (64 if gaps == 'hold' else 2) and np.isnan(col[7])
    assert col[6] == 0.0 and lay[6] == (5 if gaps == 'hold' else 2) and np.isfinite(col[1:7]).all() and col[2] != 0.0
    # the integral on its own gives the same from the device's max planes
    got = context().composite_fields({'ZH': v[order].astype(F32)[None, :]}, dist, mid[layer[order]][None, :], [90.0], spec)
    alone, n = c.column_of(spec, got['values']['ZH']['max'])
    same_bits(got['column']['ZH'], alone, 'column_of')
    same_bits(got['column_layers']['ZH'], n, 'column_of layers')


def test_refusals_leave_the_pass_and_the_context_usable():
    import ctypes as C
    rng = np.random.default_rng(17)
    c, ctx = CP(), context()
    spec = layered('3x2', 2, column={'ZH': TABLE2}, fields=('ZH',))
    plain = c.Composite('ZH', *GRIDS['3x2'])
    az, dist, heights = geometry(rng, 2, 40, '3x2', spec.z_edges)
    f = {'ZH': values(rng, (2, 40))}
    want = c.finish(c.compose(spec, f, dist, heights, az))
    assert ctx.composite_fields(f, dist, heights, az, spec, phase=1) is None                  # a pass is open
    down = np.array([500.0, 100.0, 0.0])
    one_v, one_f = np.array([1.0], F32), np.array([1.0])
    many_v, many_f = np.arange(1025, dtype=F32), np.arange(1025.0)

    def table(n, tv, tf):
        def change(s):
            s.n_table[0], s.table_v[0], s.table_f[0] = n, tv.ctypes.data, tf.ctypes.data
        return change
    tampered = {
        'n_z must lie in 0 ... 64': lambda s: setattr(s, 'n_z', 65),
        'not strictly ascending after rounding': lambda s: setattr(s, 'edges_z', down.ctypes.data),
        'COLUMN needs height layers': lambda s: setattr(s, 'n_z', 0),
        'height layers with LOWEST': lambda s: setattr(s, 'products', 67),
        'needs 2 ... 1024 breakpoints': table(1, one_v, one_f),
        'needs 2 ... 1024 breakpoints ': table(1025, many_v, many_f),
        'needs column and column_layers': lambda s: s.column.__setitem__(0, None),
        'needs column and column_layers ': lambda s: s.column_layers.__setitem__(0, None),
        'gaps differ from the open pass': lambda s: setattr(s, 'gaps', 1),
        'products must name': lambda s: setattr(s, 'products', 97),
    }
    for word, change in tampered.items():
        with pytest.raises(ValueError, match=word.strip()):
            ctx.composite_fields(f, dist, heights, az, spec, phase=2, tamper=change)
    # a later call of the pass with other edges or another table value, and a plain call, are refused like other thresholds
    other = np.array([-50.0, 360.0, 771.0])
    with pytest.raises(ValueError, match='height layers differ'):
        ctx.composite_fields(f, dist, heights, az, spec, phase=0, tamper=lambda s: setattr(s, 'edges_z', other.ctypes.data))
    with pytest.raises(ValueError, match='column table differs'):
        ctx.composite_fields(f, dist, heights, az, layered('3x2', 2, column={'ZH': (TABLE2[0], TABLE2[1] + 1.0)}, fields=('ZH',)), phase=0)
    with pytest.raises(ValueError, match='differ'):
        ctx.composite_fields(f, dist, heights, az, plain, phase=0)
    # the refusals queued nothing and left the pass as it was: it finishes with the maps of its one call
    compare(ctx.composite_fields({'ZH': np.full((2, 40), np.nan, F32)}, dist, heights, az, spec, phase=2), want, spec, 'after the refusals')
    with pytest.raises(ValueError, match='no pass open'):
        ctx.composite_fields(f, dist, heights, az, spec, phase=0)
    # ... and a plain composite behind all that is what it was
    got = ctx.composite_fields(f, dist, heights, az, plain)
    pw = c.finish(c.compose(plain, f, dist, heights, az))
    same(got['values']['ZH']['max'], pw['values']['ZH']['max'], 'plain')
    same(got['count']['ZH'], pw['count']['ZH'], 'plain count')
    assert sorted(got) == ['count', 'values'] and C.sizeof(C.c_void_p) == 8
