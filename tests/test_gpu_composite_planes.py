"""Network composites on the GPU, the kernels alone (k_comp in its gate-plane form, k_comp_merge and k_comp_finish through
cpol_debug_read "composite_fields"): hand-built rows no sweep produces, every plane against composite.compose / composite.finish
of the same rows.  Every result is a maximum, a minimum or a count of integers and the cell of a gate is found by comparisons
alone, so every comparison here is exact (NaNs positionally equal), and it is made for BOTH lane forms of k_comp: lanes that share
a cell combined inside the wavefront (1) and every lane on its own (2).

S = the gates a workgroup owns (composite.STRETCH, checked against the library)."""
import itertools

import numpy as np
import pytest

from test_gpu_composite import CP, F32, GRIDS, _ops, compare, context, geometry, stretch, values

pytestmark = pytest.mark.gpu

nan, inf = np.nan, np.inf


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def spec_on(x_edges, y_edges, products=('max', 'lowest', 'echo_top'), plane='geographic', **kw):
    if 'echo_top' in products:
        kw.setdefault('thresholds', {'ZH': [-1.0, 0.0, 0.75, 3.0], 'ATT_V': [0.0]})
    return CP().Composite(['ZH', 'ATT_V'], x_edges, y_edges, products=products, plane=plane, **kw)


def coordinates(rng, n_rays, n_gates, x_edges, y_edges):
    """Per-gate x and y inside the grid, outside it both ways, exactly on its edges, NaN, +-inf and -0.0; heights with ties, both
    zeros, a denormal, NaN."""
    out = []
    for e in (np.asarray(x_edges, dtype=np.float64), np.asarray(y_edges, dtype=np.float64)):
        span = e[-1] - e[0]
        a = rng.uniform(e[0] - 0.15 * span, e[-1] + 0.15 * span, (n_rays, n_gates))
        on = rng.random(a.shape) < 0.25
        a[on] = rng.choice(e, int(on.sum()))                                     # exactly on an edge, the last one too
        odd = rng.random(a.shape) < 0.12
        a[odd] = rng.choice(np.array([nan, inf, -inf, -0.0, 0.0]), int(odd.sum()))
        out.append(a)
    heights = rng.choice(np.array([-0.0, 0.0, 1e-45, 250.0, 1000.0, 1000.0, 2500.0, 4000.0, nan, inf], dtype=F32), (n_rays, n_gates))
    return (out[0], out[1]), heights


def check(fields, heights, xy, spec, rpb=0, tag='', forms=(1, 2), source=0):
    want = CP().finish(CP().compose(spec, fields, None, heights, None, rays_per_block=rpb, gate_xy=xy, source=source))
    for form in forms:
        got = context().composite_fields(fields, None, heights, None, spec, rpb, lane_form=form, gate_xy=xy, source=source)
        compare(got, want, spec, (tag, 'form', form))
    return want


@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_gate_plane_every_stretch_length_ray_count_grid_and_block_shape(grid):
    S = stretch()
    rng = np.random.default_rng(21)
    ex, ey = GRIDS[grid]
    spec = spec_on(ex, ey)
    counted = 0
    for n_gates in (1, 63, 64, 65, S - 1, S, S + 1):
        for n_rays in (1, 3):
            xy, heights = coordinates(rng, n_rays, n_gates, ex, ey)
            one = {k: values(rng, (n_rays, n_gates)) for k in spec.fields}
            counted += int(check(one, heights, xy, spec, 0, '%s gates %d rays %d' % (grid, n_gates, n_rays))['count']['ZH'].sum())
            # two members over one geometry: one block of all rows, and n_rows / n_rays blocks
            two = {k: values(rng, (2 * n_rays, n_gates)) for k in spec.fields}
            for rpb in (0, n_rays):
                check(two, heights, xy, spec, rpb, '%s gates %d rays %d members 2 rpb %d' % (grid, n_gates, n_rays, rpb))
    assert counted > 1000, counted


def test_gate_plane_coordinates_on_the_edges_outside_nan_inf_and_negative_zero():
    spec = CP().Composite('ZH', [0.0, 1.0, 2.0], [0.0, 1.0], products=('max', 'lowest'), plane='geographic')       # two cells
    x = np.array([[0.0, -0.0, 1.0, 2.0, np.nextafter(2.0, 0.0), -1e-300, nan, 0.5, inf, -inf, 0.5, 1.5, -5.0, 7.0, 0.5, 0.5]])
    y = np.array([[0.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, nan, 0.5, 0.5, 1.0, np.nextafter(1.0, 0.0), 0.5, 0.5, -3.0, 3.0]])
    v = np.arange(1, 17, dtype=F32)[None, :]
    h = np.full((1, 16), 100.0, dtype=F32)
    want = check({'ZH': v}, h, (x, y), spec, tag='by hand')
    # cell 0: gates 0, 1 (-0.0 lies on the edge 0.0); cell 1: gates 2, 4, 11; the last edges, NaN, the infinities and the gates
    # beyond the grid on either side of either axis do not count
    assert want['count']['ZH'].tolist() == [[[2, 3]]] and want['values']['ZH']['max'].tolist() == [[[2.0, 12.0]]]
    # every gate NaN in one coordinate, or all outside: empty maps
    for xy in ((np.full_like(x, nan), y), (x, np.full_like(y, nan)), (x + 10.0, y), (x, y - 10.0)):
        assert not check({'ZH': v}, h, xy, spec, tag='empty')['count']['ZH'].any()
    # dist is not read on a gate plane: a hook call that supplies NaN distances gives the same maps
    got = context().composite_fields({'ZH': v}, np.full((1, 16), nan, dtype=F32), h, None, spec, gate_xy=(x, y))
    compare(got, want, spec, 'NaN distances')


def test_host_made_radar_coordinates_as_a_gate_plane_give_the_radar_planes_bits():
    S = stretch()
    C, ctx = CP(), context()
    rng = np.random.default_rng(22)
    ex, ey = GRIDS['3x2']
    kw = dict(products=('max', 'lowest', 'echo_top'), thresholds={'ZH': [-1.0, 0.0, 0.75, 3.0], 'ATT_V': [0.0]}, height_range=(0.0, 4000.0))
    radar = C.Composite(['ZH', 'ATT_V'], ex, ey, **kw)
    plane = C.Composite(['ZH', 'ATT_V'], ex, ey, plane='geographic', **kw)
    for n_rays, n_gates in ((3, 65), (2, S + 1)):
        az, dist, heights = geometry(rng, n_rays, n_gates, ex, ey)
        rs, rc = C.ray_tables(az)
        xy = (dist.astype(np.float64) * rs[:, None], dist.astype(np.float64) * rc[:, None])
        f = {k: values(rng, (2 * n_rays, n_gates)) for k in radar.fields}
        for rpb in (0, n_rays):
            for form in (1, 2):
                on_radar = ctx.composite_fields(f, dist, heights, az, radar, rpb, lane_form=form)
                on_gates = ctx.composite_fields(f, None, heights, None, plane, rpb, lane_form=form, gate_xy=xy)
                compare(on_gates, on_radar, radar, ('equivalence', n_rays, n_gates, rpb, form))
                assert int(on_radar['count']['ZH'].sum()) > 10


def source_calls(rng, spec, shapes, one_cell):
    """Calls with the sources (2, 0, 1) over shared cells, values and heights from a small pool: [(fields, heights, xy, source)]."""
    ex, ey = spec.x_edges, spec.y_edges
    calls = []
    for (n_rays, n_gates), source in zip(shapes, (2, 0, 1)):
        if one_cell:
            xy = (rng.uniform(ex[0], ex[1] * 0.999, (n_rays, n_gates)), rng.uniform(ey[0], ey[1] * 0.999, (n_rays, n_gates)))
        else:
            xy = (rng.uniform(ex[0] - 1.0, ex[-1] + 1.0, (n_rays, n_gates)), rng.uniform(ey[0] - 1.0, ey[-1] + 1.0, (n_rays, n_gates)))
            xy[0][0, 0] = nan
        f = {k: rng.choice(np.array([0.75, 1.5, 2.25, -0.0, nan], dtype=F32), (n_rays, n_gates)) for k in spec.fields}
        heights = rng.choice(np.array([250.0, 1000.0, 2500.0], dtype=F32), (n_rays, n_gates))
        calls.append((f, heights, xy, source))
    return calls


def ties_and_raises(spec, calls, field='ZH'):
    """From the rule: the cells whose final MAX state is held by more than one call, and those where a later call of the list
    holds a greater state than an earlier one."""
    C = CP()
    single = [C.compose(spec, f, None, h, None, gate_xy=xy, source=s)['fields'][field]['max'] for f, h, xy, s in calls]
    final = np.maximum.reduce(single)
    holders = sum(((s == final) & (final != 0)).astype(int) for s in single)
    raised = np.zeros(final.shape, dtype=bool)
    for i in range(len(calls)):
        for j in range(i + 1, len(calls)):
            raised |= (single[i] != 0) & (single[i] < single[j])
    return int((holders > 1).sum()), int(raised.sum())


@pytest.mark.parametrize('layout', ['shared cells', 'one cell'])
def test_source_three_calls_in_every_order(layout):
    S = stretch()
    C, ctx = CP(), context()
    rng = np.random.default_rng(23)
    one_cell = layout == 'one cell'
    ex, ey = ([0.0, 1e6], [0.0, 1e6]) if one_cell else GRIDS['3x2']
    spec = spec_on(ex, ey, products=('max', 'lowest', 'echo_top', 'source'))
    if one_cell:
        # a tie of the single cell's state across calls is not left to chance: the winning gate of call 0 (source 2) is planted in call 1 (source 0)
        shapes = ((2, S + 1), (1, 65), (3, 64))
        calls = source_calls(rng, spec, shapes, True)
        for k in spec.fields:
            for c in (0, 1):
                calls[c][0][k][0, 0] = F32(3.0)
        for c in (0, 1):
            calls[c][1][0, 0] = F32(4000.0)
            calls[c][1][0, 1] = F32(100.0)          # ... and the lowest gate likewise
            for k in spec.fields:
                calls[c][0][k][0, 1] = F32(-3.0)
    else:
        # few gates per cell, so that a call often lacks the greatest value of the pool: ties and late raises both occur
        shapes = ((2, 9), (1, S + 1), (3, 7))
        calls = source_calls(rng, spec, shapes, False)
        calls[1][0]['ZH'][:, 16:] = nan
        calls[1][0]['ATT_V'][:, 24:] = nan
    ties, raises = ties_and_raises(spec, calls)
    if one_cell:
        assert ties == 1, ties
    else:
        assert ties >= 1 and raises >= 1, (ties, raises)
    state = None
    for f, h, xy, s in calls:
        state = C.compose(spec, f, None, h, None, state=state, gate_xy=xy, source=s)
    want = C.finish(state)
    if one_cell:
        assert want['values']['ZH']['source_of_max'].tolist() == [[[0.0]]] and want['values']['ZH']['source_of_lowest'].tolist() == [[[0.0]]]
    else:
        seen = want['values']['ZH']['source_of_max']
        assert len(set(seen[~np.isnan(seen)].tolist())) >= 2
    for form in (1, 2):
        for order in itertools.permutations(range(3)):
            got = None
            for n, i in enumerate(order):
                f, h, xy, s = calls[i]
                got = ctx.composite_fields(f, None, h, None, spec, phase=(1 if n == 0 else 0) | (2 if n == 2 else 0), lane_form=form,
                                           gate_xy=xy, source=s)
            compare(got, want, spec, (layout, 'form', form, 'order', order))


def test_source_with_blocks_and_on_the_radar_plane():
    """SOURCE does not need a gate plane: two calls of an ensemble shape (a block per member) on the radar plane."""
    C, ctx = CP(), context()
    rng = np.random.default_rng(24)
    ex, ey = GRIDS['3x2']
    spec = C.Composite(['ZH', 'ATT_V'], ex, ey, products=('max', 'lowest', 'source'))
    az, dist, heights = geometry(rng, 3, 70, ex, ey)
    calls = [({k: rng.choice(np.array([0.75, 1.5, nan], dtype=F32), (6, 70)) for k in spec.fields}, s) for s in (5, 4)]
    state = None
    for f, s in calls:
        state = C.compose(spec, f, dist, heights, az, state=state, rays_per_block=3, source=s)
    want = C.finish(state)
    assert set(np.unique(want['values']['ZH']['source_of_max'][~np.isnan(want['values']['ZH']['source_of_max'])]).tolist()) == {4.0, 5.0}
    for form in (1, 2):
        for order in ((0, 1), (1, 0)):
            for n, i in enumerate(order):
                got = ctx.composite_fields(calls[i][0], dist, heights, az, spec, 3, phase=1 << n, lane_form=form, source=calls[i][1])
            compare(got, want, spec, ('blocks', form, order))


def test_a_pass_without_source_after_a_source_pass_is_unaffected():
    C, ctx = CP(), context()
    rng = np.random.default_rng(25)
    ex, ey = GRIDS['3x2']
    with_source = spec_on(ex, ey, products=('max', 'lowest', 'echo_top', 'source'))
    plain = spec_on(ex, ey)
    xy, heights = coordinates(rng, 3, 130, ex, ey)
    f = {k: values(rng, (3, 130)) for k in plain.fields}
    check(f, heights, xy, with_source, tag='the SOURCE pass', source=9)
    # the same rows without SOURCE, then other rows on a larger state: neither sees what the SOURCE pass left behind it
    check(f, heights, xy, plain, tag='after the SOURCE pass')
    big = spec_on(*GRIDS['1023x1'])
    xy2, h2 = coordinates(rng, 2, 300, *GRIDS['1023x1'])
    check({k: values(rng, (2, 300)) for k in big.fields}, h2, xy2, big, tag='a larger state after the SOURCE pass')
    check(f, heights, xy, with_source, tag='a SOURCE pass again', source=0)


def test_the_plane_store_keeps_tagged_coordinates():
    ctx = context()
    rng = np.random.default_rng(26)
    ex, ey = GRIDS['3x2']
    spec = spec_on(ex, ey, products=('max',))
    xy, heights = coordinates(rng, 2, 40, ex, ey)
    other, _ = coordinates(rng, 2, 40, ex, ey)
    f = {k: values(rng, (2, 40)) for k in spec.fields}
    want = CP().finish(CP().compose(spec, f, None, heights, None, gate_xy=xy))
    want_other = CP().finish(CP().compose(spec, f, None, heights, None, gate_xy=other))
    tag = 0x7E57000000000001
    up0, hit0 = ctx.composite_plane()
    compare(ctx.composite_fields(f, None, heights, None, spec, gate_xy=xy), want, spec, 'untagged')
    assert ctx.composite_plane() == (up0, hit0)                       # (no tag: a copy per call, nothing kept)
    seen = []
    for v, coords, w in ((tag, xy, want), (tag + 1, other, want_other), (tag, xy, want), (tag + 1, other, want_other), (tag, xy, want)):
        compare(ctx.composite_fields(f, None, heights, None, spec, gate_xy=coords, plane_version=v), w, spec, ('tag', v))
        seen.append(ctx.composite_plane())
    assert seen == [(up0 + 1, hit0), (up0 + 2, hit0), (up0 + 2, hit0 + 1), (up0 + 2, hit0 + 2), (up0 + 2, hit0 + 3)], seen
    # the tag is the caller's word that the arrays did not change: under a known tag the kept copy is read, not the arrays
    compare(ctx.composite_fields(f, None, heights, None, spec, gate_xy=other, plane_version=tag), want, spec, 'the kept copy')
    # another gate count under the same tag is another plane
    f1 = {k: v[:, :39] for k, v in f.items()}
    xy1 = (np.ascontiguousarray(xy[0][:, :39]), np.ascontiguousarray(xy[1][:, :39]))
    compare(ctx.composite_fields(f1, None, heights[:, :39], None, spec, gate_xy=xy1, plane_version=tag),
            CP().finish(CP().compose(spec, f1, None, heights[:, :39], None, gate_xy=xy1)), spec, 'another shape')


def test_new_refusals_leave_the_pass_and_the_context_usable():
    C, ctx = CP(), context()
    rng = np.random.default_rng(27)
    ex, ey = GRIDS['3x2']
    spec = spec_on(ex, ey, products=('max', 'lowest', 'echo_top', 'source'), height_range=(0.0, 4000.0))
    xy, heights = coordinates(rng, 4, 70, ex, ey)
    f = {k: values(rng, (4, 70)) for k in spec.fields}

    def part(a, b):
        return ({k: v[a:b] for k, v in f.items()}, None, heights[a:b], None, spec), (np.ascontiguousarray(xy[0][a:b]), np.ascontiguousarray(xy[1][a:b]))

    state = C.compose(spec, part(0, 1)[0][0], None, heights[0:1], None, gate_xy=part(0, 1)[1], source=3)
    whole = C.finish(C.compose(spec, part(1, 4)[0][0], None, heights[1:4], None, state=state, gate_xy=part(1, 4)[1], source=1))

    def setter(**kw):
        def change(c):
            for name, v in kw.items():
                setattr(c, name, v)
        return change

    refused = [(setter(plane=2), 'plane must be'), (setter(plane=-1), 'plane must be'), (setter(gate_x=None), 'gate_x or gate_y'),
               (setter(gate_y=None), 'gate_x or gate_y'), (setter(source=255), '0 ... 254'), (setter(source=-1), '0 ... 254'),
               (setter(plane=0), 'ray_sin'), (setter(products=7), 'non-zero source without SOURCE'),
               (setter(products=7, source=0), 'differ from the open pass'), (setter(products=20, source=0), 'SOURCE needs MAX or LOWEST'),
               (setter(products=8), 'products'), (setter(products=32 | 23), 'products')]
    args, gxy = part(0, 1)
    ctx.composite_fields(*args, phase=1, gate_xy=gxy, source=3)
    args, gxy = part(1, 4)
    for change, word in refused:
        with pytest.raises(ValueError, match=word):
            ctx.composite_fields(*args, phase=2, gate_xy=gxy, source=1, tamper=change)
    # the plane differs from the open pass: the same spec on the radar plane
    radar = C.Composite(['ZH', 'ATT_V'], ex, ey, products=('max', 'lowest', 'echo_top', 'source'),
                        thresholds={'ZH': [-1.0, 0.0, 0.75, 3.0], 'ATT_V': [0.0]}, height_range=(0.0, 4000.0))
    with pytest.raises(ValueError, match='plane differs from the open pass'):
        ctx.composite_fields(args[0], np.ones((3, 70), dtype=F32), args[2], [0.0, 1.0, 2.0], radar, phase=0)
    # the pass finishes as if none of them had been made
    compare(ctx.composite_fields(*args, phase=2, gate_xy=gxy, source=1), whole, spec, 'after the refusals')
    with pytest.raises(ValueError, match='no pass open'):
        ctx.composite_fields(*args, phase=2, gate_xy=gxy, source=1)
    # the state limit counts what SOURCE adds: 1023 x 1023 cells, 13 blocks, 3 fields pass without SOURCE (979 MB of state is
    # not allocated here: the call below is the refused one), not with it; the context stays usable
    big = C.Composite(['ZH', 'ZV', 'ZDR'], np.arange(1024.0), np.arange(1024.0), products=('max', 'lowest', 'source'))
    rows = {k: np.zeros((13, 1), dtype=F32) for k in big.fields}
    with pytest.raises(ValueError, match='1 GiB'):
        ctx.composite_fields(rows, np.zeros((1, 1), dtype=F32), np.zeros((1, 1), dtype=F32), [0.0], big, rays_per_block=1, phase=1)
    args, gxy = part(0, 4)
    compare(ctx.composite_fields(*args, gate_xy=gxy, source=7), C.finish(C.compose(spec, f, None, heights, None, gate_xy=xy, source=7)), spec,
            'after the limit')
