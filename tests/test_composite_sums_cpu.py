"""The exact sums of the composites without a GPU (the product 'sum', cpol_composite_sums): the spec and its refusals, the rule
(cosmo_pol_amd/composite.py: `compose`, `finish`, `mean_of`) against math.fsum cell by cell on hand-built rows, the independence
of the result from the cut of the pass, the order of the rays and the block cut, the ctypes mirror against the header as gcc
sees it, and the host validation header (cosmo_pol_amd/csrc/cpol_comp.h) through tests/c_host/comp_check_sums.cpp, built with
the address and undefined-behaviour sanitizers and run as a program of its own.  All comparisons are exact, NaNs positionally
equal.

The rows lie on a gate plane with unit cells from 0: a gate at x = j + 0.5, y = 0.5 lies in cell j."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import objects as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
nan, inf = np.nan, np.inf
FLT_MAX = float(np.finfo(F32).max)

# the cells of the hand-built row: what each one holds
CELLS = [
    [1e30, 1.0, -1e30],                                            # exact sum 1.0; float64 in gate order gives 0.0
    [1e-45, -1e-45, 1e-45, 0.0, -0.0, 1e-39, -3e-39],              # denormals and both zeros
    [2.0 ** -149, 2.0 ** -126, 2.0 ** -100, 2.0 ** -50, 1.0, 2.0 ** 50, 2.0 ** 100, 2.0 ** 127, FLT_MAX, -2.0 ** 60, 3.1415927],
    [3.5, -3.5, 1e20, -1e20, 2.0 ** -140, -2.0 ** -140],           # an exact cancellation: +0.0
    [inf, 2.0, -inf, 5.0],                                         # +-inf is skipped and still counts
    [nan, nan],                                                    # NaN does not count: an empty cell
    [inf],                                                         # every counting gate skipped: NaN, count 1
    [-0.0],                                                        # the exact sum is zero: +0.0
    [FLT_MAX] * 9 + [-FLT_MAX] * 4,                                # beyond float32, well inside float64
    [],                                                            # no gate at all
]
# a table whose f overflows float32 between its breakpoints: f(1.2) = 2e38 is finite in float32, f(1.5) = 5e38 and the cap 1e39 are not
OVERFLOW_TABLE = (np.array([1.0, 2.0], dtype=F32), np.array([0.0, 1e39]))
# a table that is not monotonic (nothing demands it), with negative values
WAVY_TABLE = (np.array([-2.0, 0.0, 0.5, 4.0, 1e10], dtype=F32), np.array([3.0, -1.25, 7.0, 1e-3, -1e30]))


def cells_row(cells=CELLS):
    """(values float32 [1, n], x, y float64 [1, n], heights float32 [1, n]) with the gates of cell j interleaved over the row."""
    v, x = [], []
    longest = max(len(c) for c in cells)
    for i in range(longest):
        for j, c in enumerate(cells):
            if i < len(c):
                v.append(c[i])
                x.append(j + 0.5)
    v = np.array([v], dtype=F32)
    x = np.array([x], dtype=np.float64)
    return v, x, np.full_like(x, 0.5), np.full(v.shape, 100.0, dtype=F32)


def spec_of(n_cells, fields='ZH', products=('max', 'sum'), **kw):
    return CP.Composite(fields, np.arange(n_cells + 1.0), [0.0, 1.0], products=products, plane='geographic', **kw)


def weight_scalar(v, table):
    """w of one value, in Python floats (float64), then one rounding to float32."""
    if table is None:
        return float(v)
    tv, tf = [float(t) for t in table[0]], [float(t) for t in table[1]]
    i = sum(1 for t in tv if t <= v) - 1
    if i < 0:
        f = 0.0
    elif i >= len(tv) - 1:
        f = tf[-1]
    else:
        t = (float(v) - tv[i]) / (tv[i + 1] - tv[i])
        d = tf[i + 1] - tf[i]
        p = t * d
        f = tf[i] + p
    with np.errstate(over='ignore'):
        return float(F32(f))


def fsum_rule(spec, field, v, x, y, h, rpb=0):
    """(sum, skipped, count) [n_blocks, n_y, n_x] of the rule through a plain loop and math.fsum; no layers."""
    ng = v.shape[-1]
    v = v.reshape(-1, ng)
    rows, n_rays = v.shape[0], x.reshape(-1, ng).shape[0]
    x, y, h = x.reshape(n_rays, ng), y.reshape(n_rays, ng), h.reshape(n_rays, ng)
    nb = rows // rpb if rpb else 1
    per = rows // nb
    ex, ey = [float(e) for e in spec.x_edges], [float(e) for e in spec.y_edges]
    terms = [[] for _ in range(nb * spec.n_y * spec.n_x)]
    count = np.zeros(len(terms), dtype=np.uint64)
    skipped = np.zeros(len(terms), dtype=np.uint32)
    for r in range(rows):
        for g in range(ng):
            val, xx, yy, hh = float(v[r, g]), float(x[r % n_rays, g]), float(y[r % n_rays, g]), float(h[r % n_rays, g])
            if val != val or xx != xx or yy != yy or hh != hh:
                continue
            ix, iy = sum(1 for e in ex if e <= xx) - 1, sum(1 for e in ey if e <= yy) - 1
            if not (0 <= ix < spec.n_x and 0 <= iy < spec.n_y):
                continue
            if spec.height_range is not None and not (float(spec.height_range[0]) <= hh < float(spec.height_range[1])):
                continue
            cell = (r // per) * spec.n_y * spec.n_x + iy * spec.n_x + ix
            count[cell] += 1
            w = weight_scalar(val, spec.weight.get(field))
            if math.isinf(w):
                skipped[cell] += 1
            else:
                terms[cell].append(w)
    total = np.array([math.fsum(t) + 0.0 if t else nan for t in terms], dtype=np.float64)
    sh = (nb, spec.n_y, spec.n_x)
    return total.reshape(sh), skipped.reshape(sh), count.reshape(sh)


def same(got, want, tag=''):
    """Bit for bit, NaNs positionally equal."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind in 'ui':
        assert np.array_equal(got, want), (tag, got, want)
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (tag, 'NaN positions', got, want)
    word = np.uint64 if got.dtype == np.float64 else np.uint32
    assert np.array_equal(np.ascontiguousarray(got).view(word)[~gn], np.ascontiguousarray(want).view(word)[~wn]), (tag, got, want)


def same_result(a, b, spec, tag=''):
    for k in spec.fields:
        same(a['sum'][k], b['sum'][k], (tag, k, 'sum'))
        same(a['sum_skipped'][k], b['sum_skipped'][k], (tag, k, 'sum_skipped'))
        same(a['count'][k], b['count'][k], (tag, k, 'count'))
        for p in spec.planes(k):
            same(a['values'][k][p], b['values'][k][p], (tag, k, p))


def rule(spec, fields, x, y, h, rpb=0, state=None):
    return CP.compose(spec, fields, None, h, None, state=state, rays_per_block=rpb, gate_xy=(x, y))


# ---------------------------------------------------------------------------------------------------- the spec
def test_the_spec_and_its_refusals():
    ex, ey = np.arange(4.0), np.arange(3.0)
    assert (CP.SUM, CP.SUM_BIT, CP.SUM_BINS, CP.SUM_MAX_GATES) == ('sum', 256, 32, 2 ** 32 - 1)
    s = CP.Composite(['ZH', 'KDP'], ex, ey, products=('sum', 'max'), weight={'ZH': OB.zr_table()})
    assert s.products == ('max', 'sum') and s.product_mask == 257 and list(s.weight) == ['ZH']
    assert s.weight['ZH'][0].dtype == F32 and s.weight['ZH'][1].dtype == np.float64
    assert s.planes('ZH') == ['max', 'height_of_max'] and 'weight={ZH: 241 points}' in repr(s)
    assert CP.Composite('ZH', ex, ey, products=('lowest', 'sum')).product_mask == 258
    assert CP.Composite('ZH', ex, ey, products=('echo_top', 'sum'), thresholds=[1.0]).product_mask == 260
    assert CP.Composite('ZH', ex, ey, products=('max', 'column', 'sum'), z_edges=[0.0, 1.0], column={'ZH': CP.vil_table()}).product_mask == 321
    assert s != CP.Composite(['ZH', 'KDP'], ex, ey, products=('sum', 'max')) and s == CP.Composite(['ZH', 'KDP'], ex, ey, products=('sum', 'max'), weight={'ZH': OB.zr_table()})
    for bad in (dict(products='sum'), dict(products=('sum', 'column')), dict(products=('max', 'sum', 'source')), dict(products=('lowest', 'source', 'sum')),
                dict(products='max', weight={'ZH': OB.zr_table()}), dict(products=('max', 'sum'), weight={'ZV': OB.zr_table()}),
                dict(products=('max', 'sum'), weight={'RVEL': OB.zr_table()}), dict(products=('max', 'sum'), weight=OB.zr_table()),
                dict(products=('max', 'sum'), weight={'ZH': ([1.0], [1.0])}), dict(products=('max', 'sum'), weight={'ZH': (np.arange(1025.0), np.arange(1025.0))}),
                dict(products=('max', 'sum'), weight={'ZH': ([1.0, 2.0], [1.0])}), dict(products=('max', 'sum'), weight={'ZH': ([1.0, nan], [1.0, 2.0])}),
                dict(products=('max', 'sum'), weight={'ZH': ([1.0, 2.0], [1.0, inf])}), dict(products=('max', 'sum'), weight={'ZH': ([1.0, 1e39], [1.0, 2.0])}),
                dict(products=('max', 'sum'), weight={'ZH': ([1.0, 1.0 + 1e-9], [1.0, 2.0])}), dict(products=('max', 'sum'), weight={'ZH': ([2.0, 1.0], [1.0, 2.0])}),
                dict(products=('max', 'sum'), weight={'ZH': 3.0})):
        with pytest.raises(ValueError):
            CP.Composite('ZH', ex, ey, **bad)
    # no monotonicity is demanded of the values
    assert CP.Composite('ZH', ex, ey, products=('max', 'sum'), weight={'ZH': WAVY_TABLE}).weight['ZH'][1][1] == -1.25


def test_a_spec_without_sum_is_what_it_was():
    ex, ey = np.arange(4.0), np.arange(3.0)
    s = CP.Composite(['ZH', 'KDP'], ex, ey, products=('max', 'echo_top'), thresholds=[1.0, 2.0], height_range=(0.0, 10.0))
    assert s.key == (('ZH', 'KDP'), ('max', 'echo_top'), ex.tobytes(), ey.tobytes(), (s.thresholds['ZH'].tobytes(), s.thresholds['KDP'].tobytes()),
                     (F32(0.0).tobytes(), F32(10.0).tobytes()))
    assert repr(s) == 'Composite(ZH+KDP, 3 x 2 cells, products=max+echo_top, thresholds={ZH: [1.0, 2.0], KDP: [1.0, 2.0]}, height_range=[0, 10))'
    assert s.product_mask == 5 and s.planes('KDP') == ['max', 'height_of_max', 'echo_top_0', 'echo_top_1'] and s.weight == {}
    assert CP.state_bytes(s, 3) == 2 * (3 * 6 * 8 * 2 + 3 * 6 * 4 * 2)
    layered = CP.Composite('ZH', ex, ey, products=('max', 'column'), z_edges=[0.0, 1.0, 2.0], column={'ZH': CP.vil_table()})
    assert layered.key[-1][0] == 'z' and CP.state_bytes(layered, 1) == 2 * 6 * 16
    # with 'sum': the same planes, 32 bins and a skipped word more per cell
    w = CP.Composite(['ZH', 'KDP'], ex, ey, products=('max', 'echo_top', 'sum'), thresholds=[1.0, 2.0], height_range=(0.0, 10.0))
    assert w.key[:-1] == s.key[:1] + (('max', 'echo_top', 'sum'),) + s.key[2:] and w.key[-1] == ('w', ())
    assert CP.state_bytes(w, 3) == CP.state_bytes(s, 3) + 2 * (3 * 6 * 256 + 3 * 6 * 4)
    assert CP.sum_shape(w, 12, 4) == (3, 2, 3) and CP.sum_shape(CP.Composite('ZH', ex, ey, products=('max', 'sum'), z_edges=[0.0, 1.0, 2.0]), 5) == (1, 2, 2, 3)
    assert CP.state_bytes(CP.Composite('ZH', ex, [0.0, 1.0], products=('max', 'sum')), 1) == 3 * 16 + 3 * 256 + 16


# ---------------------------------------------------------------------------------------------------- the rule against math.fsum
def test_the_cells_against_fsum():
    v, x, y, h = cells_row()
    spec = spec_of(len(CELLS))
    res = CP.finish(rule(spec, {'ZH': v}, x, y, h))
    want, skipped, count = fsum_rule(spec, 'ZH', v, x, y, h)
    same(res['sum']['ZH'], want, 'sum')
    same(res['sum_skipped']['ZH'], skipped, 'skipped')
    same(res['count']['ZH'], count, 'count')
    got = res['sum']['ZH'][0, 0]
    # the naive float64 sum in gate order loses the 1.0; the exact sum keeps it
    naive = np.float64(0.0)
    for t in CELLS[0]:
        naive = naive + np.float64(F32(t))
    assert naive == 0.0 and np.sum(np.array(CELLS[0], dtype=F32).astype(np.float64)) == 0.0 and got[0] == 1.0
    assert got[3] == 0.0 and not np.signbit(got[3]) and got[7] == 0.0 and not np.signbit(got[7])
    assert got[4] == 7.0 and list(res['sum_skipped']['ZH'][0, 0][[4, 6]]) == [2, 1] and list(res['count']['ZH'][0, 0][[4, 5, 6, 9]]) == [4, 0, 1, 0]
    assert np.isnan(got[5]) and np.isnan(got[6]) and np.isnan(got[9])
    assert got[8] == 5.0 * FLT_MAX and got[8] > FLT_MAX
    assert got[1] == math.fsum(float(F32(t)) for t in CELLS[1]) and got[2] == math.fsum(float(F32(t)) for t in CELLS[2])
    # the mean: one float64 division, NaN where nothing was summed
    mean = CP.mean_of(res, 'ZH')
    assert mean.dtype == np.float64 and mean.shape == got[None, None].shape
    for j in range(len(CELLS)):
        n = int(count[0, 0, j]) - int(skipped[0, 0, j])
        if n:
            assert mean[0, 0, j] == got[j] / np.float64(n), j
        else:
            assert np.isnan(mean[0, 0, j]), j
    with pytest.raises(ValueError):
        CP.mean_of(res, 'ZV')
    with pytest.raises(ValueError):
        CP.mean_of({'count': res['count']}, 'ZH')


@pytest.mark.parametrize('table', ['overflow', 'wavy', 'zr'])
def test_weight_tables_against_fsum(table):
    tab = {'overflow': OVERFLOW_TABLE, 'wavy': WAVY_TABLE, 'zr': OB.zr_table()}[table]
    rng = np.random.default_rng(3)
    tv = tab[0]
    pool = np.concatenate([tv[:8], tv[-3:], np.nextafter(tv[:4], F32(inf)), np.nextafter(tv[:4], F32(-inf)),
                           np.array([nan, inf, -inf, 0.0, -0.0, 1e-45, 1.2, 1.5, 1.75, 3e38, -5.0, 0.25, 123.456], dtype=F32)]).astype(F32)
    v = rng.choice(pool, (3, 40)).astype(F32)
    x = rng.uniform(-0.5, 4.5, (3, 40))
    y = np.full_like(x, 0.5)
    h = np.full(v.shape, 10.0, dtype=F32)
    spec = spec_of(4, weight={'ZH': tab})
    res = CP.finish(rule(spec, {'ZH': v}, x, y, h))
    want, skipped, count = fsum_rule(spec, 'ZH', v, x, y, h)
    same(res['sum']['ZH'], want, 'sum')
    same(res['sum_skipped']['ZH'], skipped, 'skipped')
    same(res['count']['ZH'], count, 'count')
    if table == 'overflow':
        assert skipped.sum() > 0 and weight_scalar(1.2, tab) == float(F32(2e38)) and math.isinf(weight_scalar(1.5, tab)) and math.isinf(weight_scalar(7.0, tab))
    # the summand is objects.weight_of's, value by value
    w = OB.weight_of(pool[pool == pool], spec.weight['ZH'])
    assert [float(t) for t in w] == [weight_scalar(float(t), tab) for t in pool[pool == pool]]


def test_two_fields_slab_and_layers():
    rng = np.random.default_rng(5)
    v = {'ZH': rng.choice(np.array(sum(CELLS, []), dtype=F32), (4, 30)), 'KDP': rng.normal(0.0, 1e3, (4, 30)).astype(F32)}
    x, y = rng.uniform(-0.3, 3.3, (4, 30)), rng.uniform(-0.2, 1.2, (4, 30))
    h = rng.choice(np.array([0.0, 400.0, 500.0, 999.0, 1000.0, 1500.0, nan], dtype=F32), (4, 30))
    slab = CP.Composite(['ZH', 'KDP'], np.arange(4.0), [0.0, 1.0], products=('lowest', 'sum'), plane='geographic', height_range=(400.0, 1000.0),
                        weight={'KDP': WAVY_TABLE})
    res = CP.finish(rule(slab, v, x, y, h))
    for k in slab.fields:
        want, skipped, count = fsum_rule(slab, k, v[k], x, y, h)
        same(res['sum'][k], want, k)
        same(res['sum_skipped'][k], skipped, k)
        same(res['count'][k], count, k)
    # layers: layer l of the layered spec is the slab [ez[l], ez[l + 1]) of a plain one
    ez = [0.0, 500.0, 1000.0, 2000.0]
    layered = CP.Composite(['ZH', 'KDP'], np.arange(4.0), [0.0, 1.0], products=('max', 'sum'), plane='geographic', z_edges=ez, weight={'KDP': WAVY_TABLE})
    res = CP.finish(rule(layered, v, x, y, h))
    assert res['sum']['ZH'].shape == (1, 3, 1, 3) == res['sum_skipped']['KDP'].shape
    for l in range(3):
        one = CP.Composite(['ZH', 'KDP'], np.arange(4.0), [0.0, 1.0], products=('max', 'sum'), plane='geographic', height_range=(ez[l], ez[l + 1]),
                           weight={'KDP': WAVY_TABLE})
        for k in layered.fields:
            want, skipped, count = fsum_rule(one, k, v[k], x, y, h)
            same(res['sum'][k][:, l], want, (k, l))
            same(res['sum_skipped'][k][:, l], skipped, (k, l))
            same(res['count'][k][:, l], count, (k, l))


# ---------------------------------------------------------------------------------------------------- independence of the result
def random_rows(rng, rows, ng, n_cells):
    pool = np.array(sum(CELLS, []) + [1e30, -1e30, 1.0, 7.25e-12, -6.5e17, 3e38, -3e38], dtype=F32)
    v = rng.choice(pool, (rows, ng)).astype(F32)
    x = rng.uniform(-0.2, n_cells + 0.2, (rows, ng))
    y = np.full_like(x, 0.5)
    h = np.full((rows, ng), 1.0, dtype=F32)
    return v, x, y, h


def test_one_call_against_three_and_permuted_rays():
    rng = np.random.default_rng(11)
    spec = spec_of(3, fields=['ZH', 'ZDR'], products=('max', 'lowest', 'sum'), weight={'ZDR': WAVY_TABLE})
    v, x, y, h = random_rows(rng, 9, 50, 3)
    f = {'ZH': v, 'ZDR': v[::-1].copy()}
    one = CP.finish(rule(spec, f, x, y, h))
    st = None
    for lo, hi in ((0, 2), (2, 3), (3, 9)):            # three calls that differ in their ray counts
        st = rule(spec, {k: a[lo:hi] for k, a in f.items()}, x[lo:hi], y[lo:hi], h[lo:hi], state=st)
    assert st['sum_gates'] == 9 * 50
    same_result(CP.finish(st), one, spec, 'three calls')
    perm = rng.permutation(9)
    same_result(CP.finish(rule(spec, {k: a[perm] for k, a in f.items()}, x[perm], y[perm], h[perm])), one, spec, 'permuted rays')
    gperm = rng.permutation(50)
    same_result(CP.finish(rule(spec, {k: a[:, gperm] for k, a in f.items()}, x[:, gperm], y[:, gperm], h[:, gperm])), one, spec, 'permuted gates')
    # the float64 sum in gate order is not that sum: the test would not pass with it
    naive = np.zeros(3)
    ix = np.floor(x).astype(int)
    ok = (v == v) & np.isfinite(v) & (ix >= 0) & (ix < 3) & (x >= 0)
    np.add.at(naive, ix[ok], v[ok].astype(np.float64))
    assert not np.array_equal(naive, one['sum']['ZH'][0, 0])


def test_member_blocks_against_separate_calls():
    rng = np.random.default_rng(13)
    spec = spec_of(4, products=('max', 'sum'), weight={'ZH': OB.zr_table()})
    n_rays, members = 4, 3
    v, _, _, _ = random_rows(rng, n_rays * members, 33, 4)
    v = np.abs(v) * F32(1e-3)
    _, x, y, h = random_rows(rng, n_rays, 33, 4)       # the geometry: n_rays rows once
    blocks = CP.finish(rule(spec, {'ZH': v}, x, y, h, rpb=n_rays))
    assert blocks['sum']['ZH'].shape == (members, 1, 4)
    for m in range(members):
        single = CP.finish(rule(spec, {'ZH': v[m * n_rays:(m + 1) * n_rays]}, x, y, h))
        same(blocks['sum']['ZH'][m:m + 1], single['sum']['ZH'], m)
        same(blocks['sum_skipped']['ZH'][m:m + 1], single['sum_skipped']['ZH'], m)
        same(blocks['count']['ZH'][m:m + 1], single['count']['ZH'], m)
    # and all members in one block: the sum of everything
    whole = CP.finish(rule(spec, {'ZH': v}, x, y, h))
    want, skipped, count = fsum_rule(spec, 'ZH', v, x, y, h)
    same(whole['sum']['ZH'], want)
    same(whole['sum_skipped']['ZH'], skipped)


def test_maps_carry_the_sums():
    spec = spec_of(2, fields=['ZH', 'KDP'], weight={'ZH': OB.zr_table()})
    m = CP.Maps(spec, phase=3, rays_per_block=2)
    m.set_plane((np.zeros((2, 5)), np.zeros((2, 5))))
    structs, keep = m.attach(N, np.zeros(2), 5, 3, False, False, (), None)
    assert isinstance(m.wide, N.CompositeSums) and structs['composite'].products == 257 and m.wide.n_weight[0] == 241 and m.wide.n_weight[3] == 0
    arr = m.arrays()
    assert [a[0] for a in arr] == ['ZH', 'KDP', 'count', ('sum', 'ZH'), ('sum', 'KDP'), ('sum_skipped', 'ZH'), ('sum_skipped', 'KDP')]
    assert arr[3][1:] == (np.float64, (3, 1, 2)) and arr[5][1:] == (np.uint32, (3, 1, 2))
    for i, (path, _, _) in enumerate(arr):
        m.bind(path, 4096 * (i + 1))
    assert structs['composite'].values[0] == 4096 and m.wide.c.count == 3 * 4096 and m.wide.sum[3] == 5 * 4096 and m.wide.sum_skipped[0] == 6 * 4096
    # the struct of the call shares the memory of the wide one
    assert C.addressof(structs['composite']) == C.addressof(m.wide)
    m.bind_device({'sum': {'ZH': 77}, 'sum_skipped': {'KDP': 78}, 'count': 79})
    assert m.wide.sum[0] == 77 and m.wide.sum_skipped[3] == 78 and m.wide.c.count == 79
    plain = CP.Maps(spec_of(2, products='max'), phase=3)
    plain.set_plane((np.zeros((2, 5)), np.zeros((2, 5))))
    plain.attach(N, np.zeros(2), 5, None, False, False, (), None)
    assert plain.wide is None and isinstance(plain.c, N.Composite) and [a[0] for a in plain.arrays()] == ['ZH', 'count']
    with pytest.raises(ValueError):
        plain.bind_device({'sum': {'ZH': 1}})


# ---------------------------------------------------------------------------------------------------- the ABI
def test_struct_layout_matches_header(tmp_path):
    names = [f for f, _ in N.CompositeSums._fields_]
    assert names == ['c', 'n_weight', 'weight_v', 'weight_f', 'sum', 'sum_skipped']
    assert [f for f, _ in N.Composite._fields_][-8:] == ['n_z', 'gaps', 'edges_z', 'n_table', 'table_v', 'table_f', 'column', 'column_layers']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){',
             'printf("cpol_composite %zu\\n", sizeof(cpol_composite));', 'printf("cpol_composite_sums %zu\\n", sizeof(cpol_composite_sums));']
    for fname in names:
        lines.append('printf("%s %%zu\\n", offsetof(cpol_composite_sums, %s));' % (fname, fname))
    lines.append('printf("enum %d %d\\n", CPOL_COMP_SUM, CPOL_COMP_COLUMN);')
    lines.append('cpol_composite_sums w; memset(&w, 0, sizeof w); printf("off %d\\n", w.n_weight[8] == 0 && w.sum[0] == NULL && (void *)&w == (void *)&w.c); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got['cpol_composite']) == C.sizeof(N.Composite) == 856                 # (cpol_composite itself has not grown)
    assert int(got['cpol_composite_sums']) == C.sizeof(N.CompositeSums)
    for fname in names:
        assert int(got[fname]) == getattr(N.CompositeSums, fname).offset, fname
    assert int(got['c']) == 0 and int(got['n_weight']) == 856 and got['off'] == '1'
    assert got['enum'].split() == [str(CP.SUM_BIT), '64'] and CP.SUM_BIT == 256


# ---------------------------------------------------------------------------------------------------- the host validation header
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('comp_sums') / 'comp_check_sums')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'comp_check_sums.cpp'),
                        '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def run(exe, *calls):
    r = subprocess.run([exe] + list(calls), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls)
    return lines


def parse(line):
    assert line.startswith('ok '), line
    head, *fields = line.split(' | ')
    t = head.split()[1:]
    out = {t[i]: int(t[i + 1]) for i in range(0, len(t), 2)}
    out['fields'] = []
    for f in fields:
        t = f.split()
        out['fields'].append({t[i]: int(t[i + 1]) for i in range(0, len(t), 2)})
    return out


def refusal(line):
    assert line.startswith('refused '), line
    return line[len('refused '):].split(' | ')[0]


def test_host_header_refusals(exe):
    cases = [('products=256', 'products: SUM stands beside'), ('products=320,nz=2', 'products: SUM stands beside'),
             ('products=273', 'products: SUM with SOURCE'), ('products=274', 'products: SUM with SOURCE'),
             ('products=257,w1=4', 'a weight table of a field that is not requested'),
             ('w0=1', 'a weight table needs 2 ... 1024 breakpoints'), ('w0=1025', 'a weight table needs 2 ... 1024 breakpoints'),
             ('w0=-3', 'a weight table needs 2 ... 1024 breakpoints'),
             ('w0=4,wv0=null', 'weight_v or weight_f is NULL'), ('w0=4,wf0=null', 'weight_v or weight_f is NULL'),
             ('w0=4,wv0=2:nan', 'a breakpoint or a value of a weight table is NaN or infinite'),
             ('w0=4,wv0=3:inf', 'a breakpoint or a value of a weight table is NaN or infinite'),
             ('w0=4,wf0=0:nan', 'a breakpoint or a value of a weight table is NaN or infinite'),
             ('w0=4,wf0=3:-inf', 'a breakpoint or a value of a weight table is NaN or infinite'),
             ('w0=4,wv0=2:2', 'the breakpoints of a weight table are not strictly ascending'),
             ('w0=4,wv0=1:9', 'the breakpoints of a weight table are not strictly ascending'),
             ('sum=0', 'a finishing call needs sum and sum_skipped for every requested field'),
             ('skip=0', 'a finishing call needs sum and sum_skipped for every requested field'),
             ('fields=0x11,sum=0', 'a finishing call needs sum and sum_skipped for every requested field'),
             # what was refused stays refused, with the words it had
             ('products=8', 'products must name MAX, LOWEST or ECHO_TOP and no other bit'), ('products=32', 'products must name MAX, LOWEST or ECHO_TOP and no other bit'),
             ('products=49', 'products must name MAX, LOWEST or ECHO_TOP and no other bit'), ('products=96', 'products must name MAX, LOWEST or ECHO_TOP and no other bit'),
             ('products=128', 'products must name MAX, LOWEST or ECHO_TOP and no other bit'), ('products=384', 'products must name MAX, LOWEST or ECHO_TOP and no other bit'),
             ('products=512', 'products must name MAX, LOWEST or ECHO_TOP and no other bit'), ('products=0', 'products must name MAX, LOWEST or ECHO_TOP and no other bit')]
    for call, why in cases:
        got = refusal(run(exe, call)[0])
        assert got.startswith(why), (call, got)
    # tables that differ from the open pass: the size, a breakpoint, a value, a table where there was none, none where there was one
    for first, then in (('w0=4', 'w0=5'), ('w0=4', 'w0=4,wv0=3:4.5'), ('w0=4', 'w0=4,wf0=1:1.25'), ('', 'w0=4'), ('w0=4', ''),
                        ('fields=3,w0=4', 'fields=3,w1=4')):
        a, b, c = run(exe, 'phase=1,' + first, 'phase=0,' + then, 'phase=2,' + first)
        assert parse(a)['open'] == 1 and refusal(b) == 'a weight table differs from the open pass' and b.endswith('open 1') and parse(c)['open'] == 0
    # a composing call need not bring the output pointers
    a, b = run(exe, 'phase=1,sum=0,skip=0', 'phase=2,sum=0')
    assert parse(a)['open'] == 1 and refusal(b).startswith('a finishing call needs sum') and b.endswith('open 1')
    # the products are part of the pass
    a, b = run(exe, 'phase=1,products=257', 'phase=2,products=1')
    assert refusal(b) == 'fields, products or block count differ from the open pass'


def test_host_header_accepts_and_sizes(exe):
    # every accepted form: beside MAX, LOWEST, ECHO_TOP, all three, with COLUMN and layers, a gate plane is the struct's affair
    for call in ('products=257', 'products=258', 'products=260,t0=2', 'products=263,t0=1,w0=2', 'products=257,nz=3', 'products=257,w0=1024',
                 'products=257,fields=0x1ff,w8=2,w0=3', 'products=257,rows=6,rpb=2'):
        assert run(exe, call)[0].startswith('ok '), call
    # the state: per field [max][count][top][bins][skipped], all in the part a begin sets to zero; LOWEST behind it
    g = parse(run(exe, 'products=263,fields=0x9,t0=3,t3=1,nx=5,ny=3,rows=4,rpb=2,w3=7')[0])
    per = 2 * 15
    assert (g['blocks'], g['cells'], g['block_cells']) == (2, 15, 15)
    f0, f3 = g['fields']
    assert (f0['field'], f0['max'], f0['count'], f0['top'], f0['sum'], f0['skip'], f0['weight']) == (0, 0, per * 8, per * 16, per * 16 + per * 12, per * 28 + per * 256, 0)
    size0 = per * 28 + per * 256 + per * 4
    assert (f3['field'], f3['max'], f3['count'], f3['top'], f3['sum'], f3['skip'], f3['weight']) == (3, size0, size0 + per * 8, size0 + per * 16, size0 + per * 16 + ((per * 4 + 7) & ~7),
                                                                                                     size0 + per * 16 + ((per * 4 + 7) & ~7) + per * 256, 7)
    assert g['zero'] == f3['skip'] + per * 4 and g['state'] == g['zero'] + 2 * per * 8 == g['total']
    spec = CP.Composite(['ZH', 'KDP'], np.arange(6.0), np.arange(4.0), products=('max', 'lowest', 'echo_top', 'sum'), thresholds={'ZH': [1.0, 2.0, 3.0], 'KDP': [1.0]})
    assert CP.state_bytes(spec, 2) == g['state']
    # an odd number of cells: the skipped words are padded to 8 bytes
    g = parse(run(exe, 'products=257,nx=3,ny=1,nz=3')[0])
    assert g['block_cells'] == 9 and g['fields'][0]['sum'] == 144 and g['fields'][0]['skip'] == 144 + 9 * 256 and g['state'] == 144 + 9 * 256 + 40
    assert CP.state_bytes(CP.Composite('ZH', np.arange(4.0), [0.0, 1.0], products=('max', 'sum'), z_edges=[0.0, 1.0, 2.0, 3.0]), 1) == g['state']
    # a struct without the bit: what it was (no sum rows, offsets -1)
    g = parse(run(exe, 'products=1,nx=3,ny=1')[0])
    assert g['state'] == 48 and g['fields'][0]['sum'] == -1 and g['fields'][0]['skip'] == -1 and g['gates'] == 0
    # the 1 GiB limit counts the bins: 1023 x 1023 cells take 276 bytes each with MAX
    limit = 'the state of all blocks and fields must be at most 1 GiB'
    assert parse(run(exe, 'products=257,nx=1023,ny=1023,rows=3,rpb=1')[0])['state'] == 3 * 1023 * 1023 * 276 + 4      # (an odd number of skipped words)
    assert refusal(run(exe, 'products=257,nx=1023,ny=1023,rows=4,rpb=1')[0]) == limit
    assert run(exe, 'products=1,nx=1023,ny=1023,rows=4,rpb=1')[0].startswith('ok ')
    assert refusal(run(exe, 'products=257,nx=1023,ny=1023,nz=64')[0]) == limit
    assert refusal(run(exe, 'products=257,nx=1023,ny=1023,nz=64,rows=1048576,rpb=1')[0]) == limit
    assert parse(run(exe, 'products=257,fields=3,nx=1000,ny=1000')[0])['state'] == 2 * 10 ** 6 * 276
    assert refusal(run(exe, 'products=257,fields=0xf,nx=1000,ny=1000')[0]) == limit


def test_host_header_counts_the_gates_of_a_pass(exe):
    big = 'rows=1048576,gates=2048'                    # 2^31 gates in one block
    a, b, c, d, e = run(exe, 'phase=1,' + big, 'phase=0,' + big, 'phase=0,rows=1,gates=2147483647', 'phase=0,rows=1,gates=1', 'phase=2,rows=1,gates=1')
    assert parse(a)['gates'] == 2 ** 31 and parse(a)['open'] == 1
    # the second call would make 2^32: refused, the pass untouched
    assert refusal(b) == 'SUM: more than 2^32 - 1 gates would fold into one block of the pass' and b.endswith('gates %d open 1' % 2 ** 31)
    assert parse(c)['gates'] == 2 ** 32 - 1 and parse(c)['open'] == 1          # exactly the limit is accepted
    assert refusal(d).startswith('SUM: more than') and d.endswith('gates %d open 1' % (2 ** 32 - 1))
    assert refusal(e).startswith('SUM: more than') and e.endswith('open 1')
    # a begin resets the counter; per block it is rows_per_block * n_gates
    a, b, c = run(exe, 'phase=1,' + big, 'phase=1,' + big, 'phase=3,rows=1,gates=5')
    assert parse(a)['gates'] == parse(b)['gates'] == 2 ** 31 and parse(c)['gates'] == 5
    a, b, c = run(exe, 'phase=1,rows=4096,rpb=1024,gates=1048576', 'phase=0,rows=4096,rpb=1024,gates=1048576', 'phase=0,rows=4096,rpb=1024,gates=2097152')
    assert parse(a)['gates'] == 2 ** 30 and parse(b)['gates'] == 2 ** 31 and refusal(c).startswith('SUM: more than')
    # without the bit nothing is counted and nothing refused
    a, b, c = run(exe, 'products=1,phase=1,' + big, 'products=1,phase=0,' + big, 'products=1,phase=2,' + big)
    assert parse(a)['gates'] == parse(b)['gates'] == parse(c)['gates'] == 0
