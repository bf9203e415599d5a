"""Gridded composites on the GPU, the kernels alone (k_comp and k_comp_finish through cpol_debug_read "composite_fields"):
hand-built rows no sweep produces, every plane against composite.compose / composite.finish of the same rows.  Every result is
a maximum, a minimum or a count of integers and the cell of a gate is found by one float64 multiplication and comparisons, so
every comparison here is exact (NaNs positionally equal), and it is made for BOTH lane forms of k_comp: lanes that share a cell
combined inside the wavefront (1) and every lane on its own (2); form 0, the one the sweeps use, is one of the two.

S = the gates a workgroup owns (composite.STRETCH, checked against the library).  An azimuth of 90 degrees has sine exactly 1,
so x = dist exactly and y = dist * 6e-17: with x edges 0, 1, 2 ... a gate at dist = j + 0.5 lies in cell j, one at dist = j on
edge j."""
import numpy as np
import pytest

from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

F32 = np.float32
_ops = {}


def context():
    if 'op' not in _ops:
        conf, luts, cubes, _, _ = case('c2_rsg')
        op = operator(conf, luts)
        load(op, cubes[0])
        _ops['op'] = op
    return _ops['op']._ctx


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def CP():
    from cosmo_pol_amd import composite
    return composite


def stretch():
    S = context().composite_stretch()
    assert S == CP().STRETCH and S % 64 == 0
    return S


def same(got, want, tag):
    """Bit for bit, NaNs positionally equal."""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.uint64:
        assert np.array_equal(got, want), (tag, int((got != want).sum()), int(got.sum()), int(want.sum()))
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (tag, 'NaN positions', int(gn.sum()), int(wn.sum()))
    g, w = np.ascontiguousarray(got).view(np.uint32)[~gn], np.ascontiguousarray(want).view(np.uint32)[~wn]
    assert np.array_equal(g, w), (tag, int((g != w).sum()))


def compare(got, want, spec, tag):
    assert sorted(got['values']) == sorted(spec.fields) == sorted(got['count']), tag
    for k in spec.fields:
        assert list(got['values'][k]) == spec.planes(k), (tag, k)
        for p in spec.planes(k):
            same(got['values'][k][p], want['values'][k][p], (tag, k, p))
        same(got['count'][k], want['count'][k], (tag, k, 'count'))


def check(fields, dist, heights, az, spec, rpb=0, tag='', forms=(1, 2)):
    want = CP().finish(CP().compose(spec, fields, dist, heights, az, rays_per_block=rpb))
    for form in forms:
        got = context().composite_fields(fields, dist, heights, az, spec, rpb, lane_form=form)
        compare(got, want, spec, (tag, 'form', form))
    return want


SPECIAL = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, 3.0, 3.0, -3.0]


def values(rng, shape, share=0.35):
    """Random values with many ties (a small pool), NaN, infinities, signed zeros and denormals."""
    x = rng.choice(np.arange(-4, 5).astype(F32) * F32(0.75), shape).astype(F32)
    where = rng.random(shape) < share
    x[where] = rng.choice(np.array(SPECIAL, dtype=F32), int(where.sum()))
    return x


def geometry(rng, n_rays, n_gates, x_edges, y_edges):
    """Azimuths of every quadrant (the first 90 degrees: x = dist), distances inside and outside the grid, on its edges and NaN;
    heights with ties, both zeros, a denormal, NaN."""
    az = rng.uniform(0.0, 360.0, n_rays)
    az[0] = 90.0
    reach = float(max(abs(x_edges[0]), abs(x_edges[-1]), abs(y_edges[0]), abs(y_edges[-1])))
    dist = rng.uniform(0.0, 1.3 * reach, (n_rays, n_gates)).astype(F32)
    on = rng.random(n_gates) < 0.3
    dist[0, on] = rng.choice(np.asarray(x_edges, dtype=F32), int(on.sum()))        # exactly on an edge (x = dist on ray 0)
    dist[rng.random(dist.shape) < 0.05] = np.nan
    heights = rng.choice(np.array([-0.0, 0.0, 1e-45, 250.0, 1000.0, 1000.0, 2500.0, 4000.0, np.nan, np.inf], dtype=F32), (n_rays, n_gates))
    return az, dist, heights


def all_products(x_edges, y_edges, **kw):
    return CP().Composite(['ZH', 'ATT_V'], x_edges, y_edges, products=('max', 'lowest', 'echo_top'),
                          thresholds={'ZH': [-1.0, 0.0, 0.75, 3.0], 'ATT_V': [0.0]}, **kw)


GRIDS = {'1x1': ([-50.0, 50.0], [-50.0, 50.0]), '3x2': ([-40.0, -5.0, 10.0, 40.0], [-30.0, 0.0, 30.0]),
         '1023x1': (np.arange(1024.0) - 511.0, [-600.0, 600.0]), '1x1023': ([-600.0, 600.0], np.arange(1024.0) - 511.0)}


@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_every_stretch_length_ray_count_grid_and_block_shape(grid):
    S = stretch()
    rng = np.random.default_rng(7)
    ex, ey = GRIDS[grid]
    spec = all_products(ex, ey)
    for n_gates in (1, 63, 64, 65, S - 1, S, S + 1):
        for n_rays in (1, 3, 5):
            az, dist, heights = geometry(rng, n_rays, n_gates, ex, ey)
            one = {k: values(rng, (n_rays, n_gates)) for k in spec.fields}
            check(one, dist, heights, az, spec, 0, '%s gates %d rays %d' % (grid, n_gates, n_rays))
            # two members over one geometry: one block of all rows, and n_rows / n_rays blocks
            two = {k: values(rng, (2 * n_rays, n_gates)) for k in spec.fields}
            for rpb in (0, n_rays):
                check(two, dist, heights, az, spec, rpb, '%s gates %d rays %d members 2 rpb %d' % (grid, n_gates, n_rays, rpb))


def test_every_ray_and_gate_in_one_cell():
    """The contention extreme: 5 x (S + 1) gates, every one in the one cell, values and heights with many ties."""
    S = stretch()
    rng = np.random.default_rng(8)
    spec = all_products([-1e6, 1e6], [-1e6, 1e6])
    n_rays, n_gates = 5, S + 1
    az = rng.uniform(0.0, 360.0, n_rays)
    dist = rng.uniform(0.0, 5e5, (n_rays, n_gates)).astype(F32)
    heights = rng.choice(np.array([100.0, 2000.0, 2000.0, 9000.0], dtype=F32), (n_rays, n_gates))
    f = {k: rng.choice(np.array([0.5, 2.0, 2.0, -1.0], dtype=F32), (n_rays, n_gates)) for k in spec.fields}
    want = check(f, dist, heights, az, spec, 0, 'one cell')
    assert int(want['count']['ZH'].sum()) == n_rays * n_gates
    assert want['values']['ZH']['max'].item() == 2.0 and want['values']['ZH']['height_of_max'].item() == 9000.0
    assert want['values']['ZH']['height_of_lowest'].item() == 100.0 and want['values']['ZH']['lowest'].item() == -1.0


def test_every_gate_in_a_cell_of_its_own():
    rng = np.random.default_rng(9)
    ex, ey = np.arange(1024.0), [-1.0, 1.0]
    spec = all_products(ex, ey)
    for n_rays in (1, 3):
        dist = np.tile(np.arange(1023, dtype=F32) + F32(0.5), (n_rays, 1))
        heights = rng.uniform(0.0, 9000.0, dist.shape).astype(F32)
        f = {k: values(rng, dist.shape, 0.1) for k in spec.fields}
        want = check(f, dist, heights, [90.0] * n_rays, spec, 0, 'own cell, rays %d' % n_rays)
        assert int(want['count']['ZH'].max()) <= n_rays and int((want['count']['ZH'] > 0).sum()) > 900


def test_runs_of_equal_cells_across_wavefronts_and_workgroups():
    """The segmented combine's edge: one ray whose gates form runs of one cell of lengths 1, 2, 63, 64, 65, ... shifted so that
    the runs begin and end on, before and behind the boundaries of wavefronts (64) and workgroups (S); gates that do not count
    inside a run cut it."""
    S = stretch()
    rng = np.random.default_rng(10)
    ex, ey = np.arange(1024.0), [-1.0, 1.0]
    spec = all_products(ex, ey)
    for shift in (0, 1, 62, 63):
        lengths = [shift] if shift else []
        while sum(lengths) < 2 * S + 130:
            lengths += [1, 2, 63, 64, 65]
        cells = np.repeat(np.arange(len(lengths)) % 1023, lengths)
        dist = (cells.astype(F32) + F32(0.5))[None, :]
        heights = rng.choice(np.array([100.0, 2000.0, 2000.0, 9000.0], dtype=F32), dist.shape)
        for share in (0.0, 0.2):
            f = {k: values(rng, dist.shape, share) for k in spec.fields}
            check(f, dist, heights, [90.0], spec, 0, 'runs, shift %d, share %g' % (shift, share))
    # ... and the same cell again after another one (A B A within a wavefront: two runs, not one)
    cells = np.array([3, 3, 7, 3, 3, 3, 7, 7, 3] * 20)
    dist = (cells.astype(F32) + F32(0.5))[None, :]
    heights = rng.uniform(0.0, 9000.0, dist.shape).astype(F32)
    f = {k: values(rng, dist.shape, 0.0) for k in spec.fields}
    want = check(f, dist, heights, [90.0], spec, 0, 'A B A')
    assert int(want['count']['ZH'][0, 0, 3]) == 120 and int(want['count']['ZH'][0, 0, 7]) == 60


def test_value_classes_edges_and_slab_bounds():
    """Ties in value and in height, +-0.0, +-inf, denormals, NaN in the field, dist or height; gates exactly on the first, an
    inner and the last edge (the last edge is outside); slab bounds hit exactly; gates outside the grid; empty cells."""
    C = CP()
    ex, ey = [0.0, 1.0, 2.0, 3.0, 4.0], [-1.0, 1.0]
    nan, inf = np.nan, np.inf
    #                 edge0 inner  last  out   out   c0    c0    c0    c1    c1    c1    c1    c2    c2    c2    c2    c2
    dist = np.array([[0.0, 2.0, 4.0, 4.5, -0.0, 0.5, 0.5, 0.5, 1.5, 1.5, 1.5, 1.5, 2.5, 2.5, nan, 2.5, 2.5]], dtype=F32)
    hgt = np.array([[500., 500., 500., 500., 700., 100., 100., 900., 0.0, -0.0, 1e-45, 50., nan, 999., 500., 1000., 2000.]], dtype=F32)
    zh = np.array([[1.0, 1.0, 1.0, 1.0, nan, 2.0, 2.0, 2.0, -0.0, 0.0, -inf, inf, 5.0, 1e-45, 5.0, -1e-45, 7.0]], dtype=F32)
    for hr in (None, (0.0, 1000.0), (100.0, 900.0), (-inf, inf)):
        spec = C.Composite(['ZH'], ex, ey, products=('max', 'lowest', 'echo_top'), thresholds=[0.0, 2.0, inf, -inf], height_range=hr)
        want = check({'ZH': zh}, dist, hgt, [90.0], spec, 0, 'classes, slab %r' % (hr,))
        v = want['values']['ZH']
        assert np.isnan(v['max'][0, 0, 3]) and want['count']['ZH'][0, 0, 3] == 0           # the last edge and beyond: empty
    # without a slab, by hand: cell 0 holds the gate on edge 0 and three ties in the value -- the greatest height wins the maximum
    spec = C.Composite(['ZH'], ex, ey, products=('max', 'lowest'))
    want = check({'ZH': zh}, dist, hgt, [90.0], spec)
    v, n = want['values']['ZH'], want['count']['ZH'][0, 0]
    assert n.tolist() == [4, 4, 4, 0]        # (dist -0.0 is ON edge 0, since -0.0 >= 0.0, but its field is NaN)
    assert (v['max'][0, 0, 0], v['height_of_max'][0, 0, 0]) == (2.0, 900.0)
    assert (v['lowest'][0, 0, 0], v['height_of_lowest'][0, 0, 0]) == (2.0, 100.0)
    # cell 1: heights -0.0 < +0.0 in the key order, so the lowest gate is the one at -0.0 (value +0.0); the maximum is +inf
    assert np.signbit(v['height_of_lowest'][0, 0, 1]) and v['lowest'][0, 0, 1] == 0.0 and not np.signbit(v['lowest'][0, 0, 1])
    assert v['max'][0, 0, 1] == inf and v['height_of_max'][0, 0, 1] == 50.0
    # cell 2 holds the inner edge's gate; its NaN height and NaN dist gates do not count
    assert (v['max'][0, 0, 2], v['height_of_max'][0, 0, 2]) == (7.0, 2000.0) and v['lowest'][0, 0, 2] == 1.0


def test_products_alone_and_together_with_one_and_four_thresholds_and_the_slab():
    C = CP()
    rng = np.random.default_rng(11)
    ex, ey = GRIDS['3x2']
    az, dist, heights = geometry(rng, 3, 130, ex, ey)
    f = {k: values(rng, (3, 130)) for k in ('ZH', 'KDP', 'ATT_V')}
    for products in (('max',), ('lowest',), ('echo_top',), ('max', 'lowest'), ('max', 'echo_top'), ('lowest', 'echo_top'),
                     ('max', 'lowest', 'echo_top')):
        for thr in ([0.75], [-1.0, 0.0, 0.75, 3.0]):
            for hr in (None, (250.0, 2500.0)):
                kw = dict(thresholds={'ZH': thr, 'KDP': thr[:1], 'ATT_V': thr}) if 'echo_top' in products else {}
                spec = C.Composite(['ZH', 'KDP', 'ATT_V'], ex, ey, products=products, height_range=hr, **kw)
                check(f, dist, heights, az, spec, 0, repr(spec))
    # the kept form of the sweeps is one of the two
    spec = all_products(ex, ey)
    check(f, dist, heights, az, spec, 0, 'kept form', forms=(0,))


def test_a_pass_cut_into_calls_of_different_shapes():
    C, S, ctx = CP(), stretch(), context()
    rng = np.random.default_rng(12)
    ex, ey = GRIDS['3x2']
    spec = all_products(ex, ey, height_range=(0.0, 4000.0))
    calls = []
    for n_rays, n_gates in ((3, 65), (1, S + 1), (5, 7)):
        az, dist, heights = geometry(rng, n_rays, n_gates, ex, ey)
        calls.append(({k: values(rng, (n_rays, n_gates)) for k in spec.fields}, dist, heights, az))
    state = None
    for f, dist, heights, az in calls:
        state = C.compose(spec, f, dist, heights, az, state=state)
    want = C.finish(state)
    for form in (1, 2):
        for i, (f, dist, heights, az) in enumerate(calls):
            got = ctx.composite_fields(f, dist, heights, az, spec, phase=(1 if i == 0 else 0) | (2 if i == 2 else 0), lane_form=form)
            assert (got is None) == (i < 2)
        compare(got, want, spec, ('pass', form))
    # with blocks every call gives the same number of them: two members of 3, 1 and 5 rays
    state = None
    for i, (f, dist, heights, az) in enumerate(calls):
        two = {k: np.concatenate([a, a[::-1]]) for k, a in f.items()}
        state = C.compose(spec, two, dist, heights, az, state=state, rays_per_block=len(az))
        got = ctx.composite_fields(two, dist, heights, az, spec, rays_per_block=len(az), phase=(1 if i == 0 else 0) | (2 if i == 2 else 0))
    compare(got, C.finish(state), spec, 'pass with blocks')
    assert got['count']['ZH'].shape[0] == 2


def test_a_finishing_call_with_no_counting_gate_is_all_nan():
    rng = np.random.default_rng(13)
    ex, ey = GRIDS['3x2']
    spec = all_products(ex, ey)
    az, dist, heights = geometry(rng, 3, 65, ex, ey)
    f = {k: np.full((3, 65), np.nan, dtype=F32) for k in spec.fields}
    want = check(f, dist, heights, az, spec, 0, 'all NaN')
    for k in spec.fields:
        assert all(np.isnan(a).all() for a in want['values'][k].values()) and not want['count'][k].any()
    # every gate outside the grid
    f = {k: values(rng, (3, 65), 0.0) for k in spec.fields}
    want = check(f, (np.abs(dist) + F32(1e4)).astype(F32), heights, az, spec, 0, 'all outside')
    assert not want['count']['ZH'].any()


def test_refusals_leave_the_pass_and_the_context_usable():
    C, ctx = CP(), context()
    rng = np.random.default_rng(14)
    ex, ey = GRIDS['3x2']
    spec = all_products(ex, ey, height_range=(0.0, 4000.0))
    az, dist, heights = geometry(rng, 4, 70, ex, ey)
    f = {k: values(rng, (4, 70)) for k in spec.fields}
    part = lambda a, b: ({k: v[a:b] for k, v in f.items()}, dist[a:b], heights[a:b], az[a:b])     # noqa: E731
    whole = C.finish(C.compose(spec, f, dist, heights, az))
    bad_edges = np.array([0.0, np.nan, 2.0, 3.0])
    desc = np.array([0.0, 2.0, 1.0, 3.0])

    def setter(**kw):
        def change(c):
            for name, v in kw.items():
                if isinstance(v, tuple):
                    getattr(c, name)[v[0]] = v[1]
                else:
                    setattr(c, name, v)
        return change

    def thr_nan(c):
        c.thresholds[0][1] = np.nan

    refused = [
        (setter(phase=4), 'phase'), (setter(fields=0), 'fields'), (setter(fields=1 << 9), 'RVEL'), (setter(fields=1 << 10), 'fields'),
        (setter(products=0), 'products'), (setter(products=8), 'products'), (setter(n_thresholds=(0, 5)), 'thresholds'),
        (setter(n_thresholds=(0, 0)), 'thresholds'), (thr_nan, 'NaN'), (setter(h_lo=4000.0), 'h_lo < h_hi'),
        (setter(h_hi=np.nan), 'h_lo < h_hi'), (setter(h_lo=4000.0 - 1e-9), 'h_lo < h_hi'), (setter(n_x=0), 'n_x'),
        (setter(n_y=1024), '1024'), (setter(edges_x=None), 'NULL'), (setter(edges_y=None), 'NULL'),
        (setter(edges_x=bad_edges.ctypes.data), 'NaN or infinite'), (setter(edges_x=desc.ctypes.data), 'ascending'),
        (setter(ray_sin=None), 'ray_sin'), (setter(ray_cos=None), 'ray_sin'), (setter(rays_per_block=-1), 'rays_per_block'),
        (setter(rays_per_block=2), 'rays_per_block'), (setter(count=None), 'count'), (setter(values=(0, None)), 'values'),
    ]
    ctx.composite_fields(*part(0, 1), spec, phase=1)
    for i, (change, word) in enumerate(refused):
        with pytest.raises(ValueError, match=word):
            ctx.composite_fields(*part(1, 4), spec, phase=2, tamper=change)
    # what differs from the open pass
    for other in (all_products(ex, ey), all_products(ex, ey, height_range=(0.0, 4001.0)), all_products(ex, [-30.0, 1.0, 30.0]),
                  C.Composite(['ZH'], ex, ey, products=('max', 'lowest', 'echo_top'), thresholds=[-1.0, 0.0, 0.75, 3.0], height_range=(0.0, 4000.0)),
                  C.Composite(['ZH', 'ATT_V'], ex, ey, products=('max', 'lowest'), height_range=(0.0, 4000.0)),
                  C.Composite(['ZH', 'ATT_V'], ex, ey, products=('max', 'lowest', 'echo_top'), thresholds={'ZH': [-1.0, 0.0, 0.75, 3.5], 'ATT_V': [0.0]},
                              height_range=(0.0, 4000.0))):
        with pytest.raises(ValueError, match='differ'):
            ctx.composite_fields(*part(1, 4), other, phase=0)
    with pytest.raises(ValueError, match='differ'):
        ctx.composite_fields(*part(1, 4), spec, rays_per_block=1, phase=0)
    with pytest.raises(ValueError, match='no input'):
        ctx.composite_fields({'ZH': f['ZH'][1:]}, dist[1:], heights[1:], az[1:], spec, phase=0, tamper=lambda c: None)
    # the pass finishes as if none of them had been made
    compare(ctx.composite_fields(*part(1, 4), spec, phase=2), whole, spec, 'after the refusals')
    # the pass is closed now
    for phase in (0, 2):
        with pytest.raises(ValueError, match='no pass open'):
            ctx.composite_fields(*part(0, 4), spec, phase=phase)
    # the state limit: 1023 x 1023 cells, 64 blocks, 9 fields, every product (far over 1 GiB); the context stays usable
    big = C.Composite(list(C.FIELDS), np.arange(1024.0), np.arange(1024.0), products=('max', 'lowest'))
    rows = {k: np.zeros((64, 1), dtype=F32) for k in C.FIELDS}
    with pytest.raises(ValueError, match='1 GiB'):
        ctx.composite_fields(rows, np.zeros((1, 1), dtype=F32), np.zeros((1, 1), dtype=F32), [0.0], big, rays_per_block=1, phase=1)
    compare(ctx.composite_fields(*part(0, 4), spec), whole, spec, 'after the limit')
