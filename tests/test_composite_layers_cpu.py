"""Height layers and the column of the gridded composites without a GPU: the spec and its refusals, the NumPy rule (`compose`,
`finish`, `column_of`) tied to the plain rule and to hand-computed numbers, `vil_table`, the ctypes mirror of the widened
cpol_composite against the header as gcc sees it, and the host validation header (cpol_comp.h) through
tests/c_host/comp_check_layers.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import neighbourhood as NB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f4, f8, u8 = np.float32, np.float64, np.uint64
EX, EY = [0.0, 1.0], [0.0, 1.0]
TAB = (np.array([1.0, 2.0, 4.0], f4), np.array([10.0, 20.0, 60.0], f8))


def layered(z=(0.0, 500.0, 1000.0, 1500.0), fields='ZH', ex=EX, ey=EY, **kw):
    return CP.Composite(fields, ex, ey, z_edges=z, **kw)


def column_spec(z=(0.0, 500.0, 1000.0, 1500.0), gaps='zero', table=TAB, ex=EX, ey=EY):
    return CP.Composite('ZH', ex, ey, products=('max', 'column'), z_edges=z, column={'ZH': table}, gaps=gaps)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same(got, want, tag=''):
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)) or (np.array_equal(np.isnan(got), np.isnan(want))
                                                      and np.array_equal(bits(got)[~np.isnan(got)], bits(want)[~np.isnan(want)])), tag


# ---------------------------------------------------------------------------------------------------- the spec
def test_spec_members_key_and_repr():
    plain = CP.Composite('ZH', EX, EY)
    assert plain.n_z == 0 and plain.z_edges is None and plain.column == {} and plain.gaps == 'zero'
    assert CP.COLUMN_BIT == 64 and CP.MAX_LAYERS == 64 and CP.MAX_TABLE == 1024
    a = layered()
    assert a.n_z == 3 and a.z_edges.dtype == f4 and a.planes('ZH') == ['max', 'height_of_max'] and a.product_mask == 1
    assert a != plain and a == layered() and hash(a) == hash(layered()) and a != layered(z=(0.0, 500.0, 1000.0, 1501.0))
    assert '3 layers' in repr(a) and 'layers' not in repr(plain)
    c = column_spec()
    assert c.product_mask == 65 and c.products == ('max', 'column') and c.column['ZH'][0].dtype == f4 and c.column['ZH'][1].dtype == f8
    assert c != a and c != column_spec(gaps='hold') and c == column_spec()
    assert c != column_spec(table=(TAB[0], np.array([10.0, 20.0, 61.0])))
    assert c != column_spec(table=(np.array([1.0, 2.0, 5.0]), TAB[1]))
    assert 'column={ZH: 3 points}' in repr(c) and 'gaps=zero' in repr(c) and 'gaps=hold' in repr(column_spec(gaps='hold'))
    # a plain spec keeps the key it had
    assert len(plain.key) == 6
    # shapes and the state
    assert CP.shape(a, 'ZH', 6, 3) == (2, 3, 2, 1, 1) and CP.count_shape(a, 6, 3) == (2, 3, 1, 1, 1) and CP.column_shape(c, 6, 3) == (2, 1, 1)
    assert CP.shape(plain, 'ZH', 6, 3) == (2, 2, 1, 1) and CP.count_shape(plain, 6, 3) == (2, 1, 1, 1)
    assert CP.state_bytes(a, 2) == 2 * 3 * 16 and CP.state_bytes(plain, 2) == 2 * 16
    big = layered(z=np.arange(65.0), fields=['ZH', 'KDP'], ex=np.arange(301.0), ey=np.arange(301.0))
    assert big.n_z == 64 and CP.state_bytes(big, 1) == 2 * 64 * 90000 * 16


def test_spec_refusals():
    bad = {
        'z_edges: 2 ... 65 edges': dict(z_edges=[0.0]),
        'z_edges: 2 ... 65 edges ': dict(z_edges=np.arange(66.0)),
        'z_edges: 2 ... 65 edges  ': dict(z_edges=[[0.0, 1.0]]),
        'an edge is NaN': dict(z_edges=[0.0, np.nan]),
        'not strictly ascending after rounding': dict(z_edges=[0.0, 2.0, 1.0]),
        'not strictly ascending after rounding ': dict(z_edges=[0.0, 1.0, 1.0]),
        'first and last edge are the slab': dict(z_edges=[0.0, 1.0], height_range=(0.0, 1.0)),
        "z_edges with 'lowest'": dict(z_edges=[0.0, 1.0], products=('max', 'lowest')),
        "z_edges with 'echo_top'": dict(z_edges=[0.0, 1.0], products=('max', 'echo_top'), thresholds=[1.0]),
        "z_edges with 'source'": dict(z_edges=[0.0, 1.0], products=('max', 'source')),
        "'column' needs z_edges": dict(products=('max', 'column'), column={'ZH': TAB}),
        "'column' needs 'max'": dict(z_edges=[0.0, 1.0], products=('column',), column={'ZH': TAB}),
        "'column' needs column =": dict(z_edges=[0.0, 1.0], products=('max', 'column')),
        "'column' needs column = ": dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={}),
        'gaps: one of zero, hold': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'ZH': TAB}, gaps='linear'),
        'not a field of the composite': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'KDP': TAB}),
        '2 ... 1024 breakpoints, got 1': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'ZH': ([1.0], [1.0])}),
        '2 ... 1024 breakpoints, got 1025': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'ZH': (np.arange(1025.0), np.arange(1025.0))}),
        '3 breakpoints and 2 values': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'ZH': ([1.0, 2.0, 3.0], [1.0, 2.0])}),
        'NaN or infinite': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'ZH': ([1.0, np.inf], [1.0, 2.0])}),
        'NaN or infinite ': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'ZH': ([1.0, 1e39], [1.0, 2.0])}),
        'NaN or infinite  ': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'ZH': ([1.0, 2.0], [1.0, np.nan])}),
        'not strictly ascending in float32': dict(z_edges=[0.0, 1.0], products=('max', 'column'), column={'ZH': ([1.0, 1.0 + 1e-9], [1.0, 2.0])}),
        "column tables without 'column'": dict(z_edges=[0.0, 1.0], column={'ZH': TAB}),
        "gaps without 'column'": dict(z_edges=[0.0, 1.0], gaps='hold'),
    }
    for word, kw in bad.items():
        with pytest.raises(ValueError, match=word.strip().replace('(', r'\(')):
            CP.Composite('ZH', EX, EY, **kw)
    # edges that differ in float64 and collide in float32
    with pytest.raises(ValueError, match='after rounding to float32'):
        layered(z=(0.0, 1000.0, 1000.00001))
    assert layered(z=(0.0, 1000.0, 1000.0001)).n_z == 2
    # the largest stack and table pass; an infinite last edge is an edge
    assert layered(z=np.arange(65.0)).n_z == 64 and layered(z=(0.0, 1e39)).z_edges[1] == np.inf
    assert len(column_spec(table=(np.arange(1024.0), np.arange(1024.0))).column['ZH'][0]) == 1024
    # a table for one of two fields is a column of that field alone
    two = CP.Composite(['ZH', 'KDP'], EX, EY, products=('max', 'column'), z_edges=[0.0, 1.0], column={'KDP': TAB})
    assert list(two.column) == ['KDP']
    # scores of a layered composite are not built
    with pytest.raises(ValueError, match='height layers is not scored'):
        NB.Fractions(layered(), 'ZH', [1.0], [1])
    # `source` stays 0
    with pytest.raises(ValueError, match="non-zero source"):
        CP.Maps(layered()).set_plane(None, 0, 1)
    with pytest.raises(ValueError, match='non-zero source'):
        CP.compose(layered(), {'ZH': np.ones((1, 1), f4)}, np.ones((1, 1), f4), np.ones((1, 1), f4), [90.0], source=1)


# ---------------------------------------------------------------------------------------------------- the layers of the rule
def one_cell(spec, heights, v=None, **kw):
    h = np.asarray(heights, f4)[None, :]
    v = np.arange(1, h.size + 1, dtype=f4)[None, :] if v is None else np.asarray(v, f4)[None, :]
    return CP.finish(CP.compose(spec, {'ZH': v}, np.full(h.shape, 0.5, f4), h, [90.0], **kw))


def test_a_gate_on_every_edge_and_special_heights():
    spec = layered(z=(-0.0, 500.0, 1000.0, 1500.0))
    below = np.nextafter(f4(500.0), f4(0.0))
    r = one_cell(spec, [0.0, 500.0, 1000.0, 1500.0])
    # on the first edge: layer 0; on an inner edge: the upper layer; on the last edge: nowhere
    assert r['count']['ZH'].ravel().tolist() == [1, 1, 1]
    assert r['values']['ZH']['max'].ravel().tolist() == [1.0, 2.0, 3.0] and r['values']['ZH']['height_of_max'].ravel().tolist() == [0.0, 500.0, 1000.0]
    assert r['values']['ZH']['max'].shape == (1, 3, 1, 1) and r['count']['ZH'].dtype == u8
    r = one_cell(spec, [below, np.nextafter(f4(1500.0), f4(0.0)), np.nextafter(f4(1500.0), f4(2000.0))])
    assert r['count']['ZH'].ravel().tolist() == [1, 0, 1] and r['values']['ZH']['max'].ravel().tolist()[::2] == [1.0, 2.0]
    # NaN, +-inf count nowhere; -0.0 lies on the first edge +0.0 (and on an edge -0.0) and counts in layer 0 with its own key
    r = one_cell(spec, [np.nan, np.inf, -np.inf, -0.0, -1e-45])
    assert r['count']['ZH'].ravel().tolist() == [1, 0, 0] and r['values']['ZH']['max'][0, 0, 0, 0] == 4.0
    assert np.signbit(r['values']['ZH']['height_of_max'][0, 0, 0, 0]) and np.isnan(r['values']['ZH']['max'][0, 1:]).all()
    # an infinite last edge takes every finite height, and not +inf
    r = one_cell(layered(z=(0.0, 1e39)), [3e38, np.inf])
    assert r['count']['ZH'].ravel().tolist() == [1]


def volume(rng, n_rays, n_gates):
    az = rng.uniform(0.0, 360.0, n_rays)
    dist = rng.uniform(0.0, 60.0, (n_rays, n_gates)).astype(f4)
    pool = np.array([-5.0, 0.0, -0.0, 249.99998, 250.0, 499.99997, 500.0, 700.0, 999.99994, 1000.0, 1200.0, np.nan, np.inf], f4)
    h = rng.choice(pool, (n_rays, n_gates))
    v = rng.choice(np.array([np.nan, -1.5, 0.0, 0.75, 0.75, 3.0, np.inf, -np.inf], f4), (2 * n_rays, n_gates))
    return az, dist, h, v


@pytest.mark.parametrize('rpb', [0, 4])
def test_layers_equal_plain_height_range_passes(rpb):
    """Ties the new rule to the old one: layer l of a layered pass is the plain composite of the slab [ez[l], ez[l + 1])."""
    rng = np.random.default_rng(3)
    ex, ey, z = [-40.0, -5.0, 10.0, 40.0], [-30.0, 0.0, 30.0], [0.0, 250.0, 500.0, 1000.0]
    az, dist, h, v = volume(rng, 4, 37)
    fields = {'ZH': v, 'KDP': v[::-1].copy()}
    spec = CP.Composite(['ZH', 'KDP'], ex, ey, z_edges=z)
    got = CP.finish(CP.compose(spec, fields, dist, h, az, rays_per_block=rpb))
    for l in range(3):
        plain = CP.Composite(['ZH', 'KDP'], ex, ey, height_range=(z[l], z[l + 1]))
        want = CP.finish(CP.compose(plain, fields, dist, h, az, rays_per_block=rpb))
        for k in spec.fields:
            for p in ('max', 'height_of_max'):
                same(got['values'][k][p][:, l], want['values'][k][p], (l, k, p))
            same(got['count'][k][:, l], want['count'][k], (l, k))
    assert got['count']['ZH'].sum() > 20 and 'column' not in got


def test_a_pass_cut_into_calls_gives_the_same_state():
    rng = np.random.default_rng(4)
    spec = column_spec(z=(0.0, 250.0, 500.0, 1000.0), ex=[-40.0, -5.0, 10.0, 40.0], ey=[-30.0, 0.0, 30.0], gaps='hold')
    az, dist, h, v = volume(rng, 6, 21)
    v = v[:6]
    whole = CP.compose(spec, {'ZH': v}, dist, h, az)
    st = None
    for lo, hi in ((0, 1), (1, 4), (4, 6)):
        st = CP.compose(spec, {'ZH': v[lo:hi]}, dist[lo:hi], h[lo:hi], az[lo:hi], state=st)
    st = CP.compose(spec, {'ZH': v[:2, :5]}, dist[:2, :5], np.full((2, 5), 5000.0, f4), az[:2], state=st)     # (hits nothing)
    for q in ('max', 'count'):
        assert np.array_equal(st['fields']['ZH'][q], whole['fields']['ZH'][q])
    a, b = CP.finish(st), CP.finish(whole)
    same(a['column']['ZH'], b['column']['ZH'])
    same(a['column_layers']['ZH'], b['column_layers']['ZH'])
    with pytest.raises(ValueError, match='differ from the state'):
        CP.compose(column_spec(z=(0.0, 250.0, 500.0, 1000.0), ex=[-40.0, -5.0, 10.0, 40.0], ey=[-30.0, 0.0, 30.0]), {'ZH': v}, dist, h, az, state=whole)


# ---------------------------------------------------------------------------------------------------- the column by hand
def planes(*layers):
    return np.array(layers, f4).reshape(1, len(layers), 1, 1)


def test_column_of_by_hand():
    nan = np.nan
    spec = column_spec()                       # layers of 500 m; table 1 -> 10, 2 -> 20, 4 -> 60
    col = lambda s, *m: tuple(a.ravel()[0] for a in CP.column_of(s, planes(*m)))
    assert col(spec, 0.5, nan, nan) == (0.0, 1)                    # below the table: no content, but a layer that counts
    assert col(spec, 1.0, nan, nan) == (10.0 * 500.0, 1)          # on a breakpoint
    assert col(spec, 2.0, 4.0, nan) == (20.0 * 500.0 + 60.0 * 500.0, 2)
    assert col(spec, 3.0, nan, nan) == ((20.0 + 0.5 * 40.0) * 500.0, 1)          # between breakpoints
    assert col(spec, 4.0, 7.0, np.inf) == (3 * 60.0 * 500.0, 3)                   # at and above the cap, +inf
    assert col(spec, -np.inf, -0.0, 0.99999994) == (0.0, 3)
    c, n = CP.column_of(spec, planes(nan, nan, nan))
    assert np.isnan(c).all() and n.ravel()[0] == 0 and c.dtype == f8 and n.dtype == np.uint8 and c.shape == (1, 1, 1)
    # one float64 operation at a time: an interpolation that is not exact, in the order of the rule
    v = f4(1.3)
    t = (f8(v) - 1.0) / (2.0 - 1.0)
    f = 10.0 + t * (20.0 - 10.0)
    assert col(spec, v, v, nan) == ((0.0 + f * 500.0) + f * 500.0, 2)
    # empty layers at the bottom, in the middle and on top, under both gaps
    five = (0.0, 100.0, 300.0, 600.0, 1000.0, 1500.0)
    zero, hold = column_spec(z=five), column_spec(z=five, gaps='hold')
    assert col(zero, nan, 1.0, nan, 2.0, nan) == (0.0 + 10.0 * 200.0 + 20.0 * 400.0, 2)
    assert col(hold, nan, 1.0, nan, 2.0, nan) == ((0.0 + 10.0 * 200.0 + 10.0 * 300.0) + 20.0 * 400.0, 3)
    assert col(hold, 1.0, nan, nan, nan, 4.0) == ((((0.0 + 10.0 * 100.0) + 10.0 * 200.0) + 10.0 * 300.0) + 10.0 * 400.0 + 60.0 * 500.0, 5)
    assert col(hold, nan, nan, 2.0, nan, nan) == (20.0 * 300.0, 1) == col(zero, nan, nan, 2.0, nan, nan)
    assert col(hold, 0.5, nan, 2.0, nan, nan) == (0.0 * 100.0 + 0.0 * 200.0 + 20.0 * 300.0, 3)              # a held layer below the table
    # dz is the difference of the ROUNDED edges in float64
    odd = column_spec(z=(0.1, 0.7))
    assert col(odd, 1.0) == (10.0 * (f8(f4(0.7)) - f8(f4(0.1))), 1)
    # several blocks and cells at once; what the function refuses
    m = np.full((2, 3, 1, 1), nan, f4)
    m[1, 2] = 2.0
    c, n = CP.column_of(spec, m)
    assert np.isnan(c[0, 0, 0]) and c[1, 0, 0] == 10000.0 and n.ravel().tolist() == [0, 1]
    with pytest.raises(ValueError, match='float32'):
        CP.column_of(spec, m.astype(f8))
    with pytest.raises(ValueError, match='float32'):
        CP.column_of(spec, m[:, :2])
    with pytest.raises(ValueError, match="no product 'column'"):
        CP.column_of(layered(), m)
    with pytest.raises(ValueError, match='no column table'):
        CP.column_of(spec, m, field='KDP')


def test_finish_carries_the_column():
    spec = column_spec(gaps='hold')
    r = one_cell(spec, [100.0, 1200.0, 1300.0], v=[2.0, 1.0, 4.0])
    assert sorted(r) == ['column', 'column_layers', 'count', 'values']
    assert r['column']['ZH'].ravel().tolist() == [20.0 * 500.0 + 20.0 * 500.0 + 60.0 * 500.0] and r['column_layers']['ZH'].ravel().tolist() == [3]
    c, n = CP.column_of(spec, r['values']['ZH']['max'])
    same(c, r['column']['ZH'])
    same(n, r['column_layers']['ZH'])


def test_vil_table():
    tv, tf = CP.vil_table()
    assert tv.dtype == f4 and tf.dtype == f8 and len(tv) == len(tf) == 265 and np.all(tv[1:] > tv[:-1])
    assert tv[0] == f4(0.1) and tv[-1] == f4(10.0 ** 5.6)
    # at the breakpoints the interpolant is the formula evaluated at the ROUNDED breakpoints, exactly as stored
    assert np.array_equal(tf, 3.44e-6 * np.power(tv.astype(f8), 4.0 / 7.0))
    spec = CP.Composite('ZH', EX, EY, products=('max', 'column'), z_edges=[0.0, 1.0], column={'ZH': (tv, tf)})
    at = np.array([CP.column_of(spec, planes(v))[0].ravel()[0] for v in tv[::13]])
    assert np.array_equal(at, tf[::13] * 1.0)
    # between them: f is concave with exponent 4 / 7, so the chord's relative error over a step of 0.25 dB is at most
    # (12 / 49) (10 ** 0.025 - 1) ** 2 / 8 = 1.075e-4
    assert (12.0 / 49.0) * (10.0 ** 0.025 - 1.0) ** 2 / 8.0 < 1.1e-4
    rng = np.random.default_rng(5)
    v = np.unique((10.0 ** rng.uniform(-1.0, 5.6, 4000)).astype(f4))
    v = v[(v > tv[0]) & (v < tv[-1])]
    got = CP.column_of(spec, v.reshape(-1, 1, 1, 1))[0].ravel()          # (one block per sample)
    want = 3.44e-6 * np.power(v.astype(f8), 4.0 / 7.0)
    rel = np.abs(got - want) / want
    assert rel.max() <= 1.1e-4 and (got <= want * (1 + 1e-12)).all()
    # the cap, and nothing below the table
    assert CP.column_of(spec, planes(1e9))[0].ravel()[0] == tf[-1] and CP.column_of(spec, planes(0.05))[0].ravel()[0] == 0.0
    # other ranges
    tv2, tf2 = CP.vil_table(0.0, 50.0, 1.0)
    assert len(tv2) == 51 and tv2[0] == 1.0 and tv2[-1] == f4(1e5)
    for bad in ((10.0, 10.0, 1.0), (0.0, 10.0, 0.0), (0.0, 100.0, 0.01)):
        with pytest.raises(ValueError, match='vil_table'):
            CP.vil_table(*bad)


# ---------------------------------------------------------------------------------------------------- the product object
def test_maps_arrays_bind_finish_and_join():
    spec = CP.Composite(['ZH', 'KDP'], np.arange(4.0), np.arange(3.0), products=('max', 'column'), z_edges=[0.0, 1.0, 2.0, 3.0, 4.0],
                        column={'KDP': TAB}, gaps='hold')
    p = CP.Maps(spec, rays_per_block=4)
    structs, keep = p.attach(N, np.arange(4.0), 5, 2, False, False, (), None)
    c = structs['composite']
    assert (c.n_z, c.gaps, c.products) == (4, 1, 65) and list(c.n_table) == [0, 0, 0, 3, 0, 0, 0, 0, 0]
    assert c.table_v[3] == spec.column['KDP'][0].ctypes.data and c.table_f[3] == spec.column['KDP'][1].ctypes.data and not c.table_v[0]
    assert np.array_equal(np.ctypeslib.as_array(C.cast(c.edges_z, C.POINTER(C.c_double)), (5,)), [0.0, 1.0, 2.0, 3.0, 4.0])
    arrays = p.arrays()
    assert [(k, np.dtype(t).name, sh) for k, t, sh in arrays] == [
        ('ZH', 'float32', (2, 4, 2, 2, 3)), ('KDP', 'float32', (2, 4, 2, 2, 3)), ('count', 'uint64', (2, 4, 2, 2, 3)),
        (('column', 'KDP'), 'float64', (2, 2, 3)), (('column_layers', 'KDP'), 'uint8', (2, 2, 3))]
    for j, (k, _, _) in enumerate(arrays):
        p.bind(k, 1000 + j)
    assert (c.values[0], c.values[3], c.count, c.column[3], c.column_layers[3]) == (1000, 1001, 1002, 1003, 1004) and not c.column[0]
    views = {k: np.zeros(sh, t) for k, t, sh in arrays}
    views['KDP'][:, :, 1] = 7.0
    views['count'][:, :, 1] = 3
    out = p.finish(views, None)
    assert sorted(out) == ['column', 'column_layers', 'count', 'values', 'x_edges', 'y_edges', 'z_edges']
    assert out['values']['KDP']['height_of_max'].shape == (2, 4, 2, 3) and (out['values']['KDP']['height_of_max'] == 7.0).all()
    assert (out['values']['KDP']['max'] == 0.0).all() and (out['count']['KDP'] == 3).all() and (out['count']['ZH'] == 0).all()
    assert list(out['column']) == ['KDP'] and out['column']['KDP'].shape == (2, 2, 3) and out['z_edges'] is spec.z_edges
    j = p.join([out, out], np.concatenate)
    assert j['column']['KDP'].shape == (4, 2, 3) and j['column_layers']['KDP'].shape == (4, 2, 3) and j['values']['ZH']['max'].shape == (4, 4, 2, 3)
    # device outputs
    p.bind_device({'values': {'ZH': 11, 'KDP': 12}, 'count': 13, 'column': {'KDP': 14}, 'column_layers': {'KDP': 15}})
    assert (c.values[0], c.values[3], c.count, c.column[3], c.column_layers[3]) == (11, 12, 13, 14, 15)
    with pytest.raises(ValueError, match='unknown entry'):
        p.bind_device({'columns': {}})
    # a plain spec: what it was
    q = CP.Maps(CP.Composite('ZH', np.arange(4.0), np.arange(3.0)))
    c = q.attach(N, np.arange(4.0), 5, None, False, False, (), None)[0]['composite']
    assert (c.n_z, c.gaps, c.edges_z) == (0, 0, None) and not any(c.n_table)
    assert [(k, sh) for k, _, sh in q.arrays()] == [('ZH', (1, 2, 2, 3)), ('count', (1, 1, 2, 3))]


# ---------------------------------------------------------------------------------------------------- the C ABI
OLD_OFFSETS = {'fields': 0, 'phase': 4, 'products': 8, 'rays_per_block': 12, 'n_x': 16, 'n_y': 20, 'use_slab': 24, 'n_thresholds': 28,
               'h_lo': 64, 'h_hi': 72, 'thresholds': 80, 'edges_x': 368, 'edges_y': 376, 'ray_sin': 384, 'ray_cos': 392, 'values': 400,
               'count': 472, 'plane': 480, 'source': 484, 'gate_x': 488, 'gate_y': 496, 'plane_version': 504}
NEW = ('n_z', 'gaps', 'edges_z', 'n_table', 'table_v', 'table_f', 'column', 'column_layers')


def test_struct_layout_matches_header(tmp_path):
    names = [f for f, _ in N.Composite._fields_]
    assert tuple(names[-len(NEW):]) == NEW and names[:len(OLD_OFFSETS)] == list(OLD_OFFSETS)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){',
             'printf("cpol_composite %zu\\n", sizeof(cpol_composite));']
    for fname in names:
        lines.append('printf("%s %%zu\\n", offsetof(cpol_composite, %s));' % (fname, fname))
    lines.append('printf("limits %d %d %d %d %d\\n", CPOL_COMP_COLUMN, CPOL_COMP_MAX_LAYERS, CPOL_COMP_MAX_TABLE, CPOL_COMP_GAPS_ZERO, CPOL_COMP_GAPS_HOLD);')
    lines.append('printf("old %d %d %d %d\\n", CPOL_COMP_MAX, CPOL_COMP_LOWEST, CPOL_COMP_ECHO_TOP, CPOL_COMP_SOURCE);')
    lines.append('cpol_composite c; memset(&c, 0, sizeof c); printf("off %d\\n", c.n_z == 0 && c.gaps == 0 && c.edges_z == NULL && c.column[8] == NULL); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got['cpol_composite']) == C.sizeof(N.Composite)
    for fname in names:
        assert int(got[fname]) == getattr(N.Composite, fname).offset, fname
    # every member that existed stays where it was
    for fname, off in OLD_OFFSETS.items():
        assert int(got[fname]) == off, fname
    assert int(got['n_z']) == 512 and got['off'] == '1'
    assert got['limits'].split() == [str(CP.COLUMN_BIT), str(CP.MAX_LAYERS), str(CP.MAX_TABLE), '0', '1'] and got['old'].split() == ['1', '2', '4', '16']
    assert CP.GAPS == ('zero', 'hold')


# ---------------------------------------------------------------------------------------------------- the host validation header
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('comp_layers') / 'comp_check_layers')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'comp_check_layers.cpp'),
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
    parts = line.split(' | ')
    w = parts[0].split()
    out = dict(zip(w[1::2], w[2::2]))
    out = {k: (float.fromhex(x) if k.startswith('ez') else int(x)) for k, x in out.items()}
    out['fields'] = {}
    for p in parts[1:]:
        q = p.split()
        out['fields'][int(q[1])] = dict(zip(q[2::2], (int(x) for x in q[3::2])))
    return out


COL = 'products=65,nz=2,tab0=3'


def test_host_header_refusals(exe):
    cases = {
        'nz=65': 'n_z must lie in 0 ... 64', 'nz=-1': 'n_z must lie in 0 ... 64',
        'nz=2,ez=0:1:1': 'not strictly ascending after rounding', 'nz=2,ez=2:1:0': 'not strictly ascending after rounding',
        'nz=2,ez=0:1000:1000.00001': 'not strictly ascending after rounding',
        'nz=1,ez=nan:1': 'a layer edge is NaN', 'nz=1,ez=0:nan': 'a layer edge is NaN', 'nz=1,ez=null': 'edges_z is NULL',
        'nz=2,slab=1': 'height layers with a height slab', 'products=3,nz=1': 'height layers with LOWEST', 'products=2,nz=1': 'height layers with LOWEST',
        'products=5,nz=1,t0=1': 'height layers with ECHO_TOP', 'products=17,nz=1': 'height layers with SOURCE',
        'products=65,tab0=3': 'COLUMN needs height layers', 'products=64,nz=2,tab0=3': 'COLUMN needs MAX',
        'products=65,nz=2': 'COLUMN needs a table', 'nz=1,tab0=2': 'a column table without COLUMN', 'tab0=2': 'a column table without COLUMN',
        'products=65,nz=1,tab1=2': 'a field that is not requested',
        'products=65,nz=2,tab0=1': 'needs 2 ... 1024 breakpoints', 'products=65,nz=2,tab0=1025': 'needs 2 ... 1024 breakpoints',
        'products=65,nz=2,tab0=-1': 'needs 2 ... 1024 breakpoints',
        COL + ',tv0=null': 'table_v or table_f is NULL', COL + ',tf0=null': 'table_v or table_f is NULL',
        COL + ',tv0=1:0.5': 'not strictly ascending', COL + ',tv0=1:1': 'not strictly ascending', COL + ',tv0=2:inf': 'NaN or infinite',
        COL + ',tv0=0:nan': 'NaN or infinite', COL + ',tf0=1:nan': 'NaN or infinite', COL + ',tf0=2:-inf': 'NaN or infinite',
        'nz=2,gaps=1': 'gaps without COLUMN', 'gaps=1': 'gaps without COLUMN', COL + ',gaps=2': 'gaps must be', COL + ',gaps=-1': 'gaps must be',
        COL + ',col=0': 'needs column and column_layers', COL + ',lay=0': 'needs column and column_layers',
        COL + ',source=1': 'non-zero source without SOURCE',
        'products=32': 'products must name', 'products=8': 'products must name', 'products=49': 'products must name', 'products=128': 'products must name',
        'products=96,nz=1': 'products must name',
        'nz=2,fr=1': 'height layers is not scored', COL + ',fr=1': 'height layers is not scored',
    }
    for call, word in cases.items():
        line, = run(exe, call)
        assert line.startswith('refused ') and word in line, (call, line)
    # the message of the product bits begins as it always did
    assert run(exe, 'products=32')[0].startswith('refused products must name MAX, LOWEST or ECHO_TOP and no other bit')
    # accepted: layers alone, the column under both gaps, a gate plane, 64 layers, 1024 breakpoints, a call that does not finish
    # without output pointers, an infinite last edge, fractions beside a plain composite
    for call in ('nz=3', COL, COL + ',gaps=1', COL + ',plane=1', 'nz=64', 'products=65,nz=1,tab0=1024', COL + ',phase=1,col=0,lay=0',
                 'nz=1,ez=0:1e39', 'fr=1', 'products=65,nz=2,fields=0x9,tab3=2'):
        assert run(exe, call)[0].startswith('ok '), call
    p = parse(run(exe, 'nz=2,ez=0.1:0.7:1e39')[0])
    assert (p['ez0'], p['ezn']) == (float(f4(0.1)), float('inf'))


def test_host_header_state_sizes_and_the_limit(exe):
    p = parse(run(exe, 'rows=12,gates=50,fields=0x9,rpb=3,nx=3,ny=2,nz=5')[0])
    assert (p['blocks'], p['cells'], p['block_cells'], p['nz'], p['column']) == (4, 6, 30, 5, 0)
    per = 4 * 30
    f0, f3 = p['fields'][0], p['fields'][3]
    assert (f0['max'], f0['count'], f3['max'], f3['count']) == (0, per * 8, per * 16, per * 24) and (f0['planes'], f3['planes']) == (2, 2)
    assert p['zero'] == p['state'] == p['total'] == per * 32
    spec = CP.Composite(['ZH', 'KDP'], np.arange(4.0), np.arange(3.0), z_edges=500.0 * np.arange(6))
    assert CP.state_bytes(spec, 4) == p['total']
    q = parse(run(exe, 'rows=12,gates=50,fields=0x9,rpb=3,nx=3,ny=2,nz=5,products=65,tab3=7,gaps=1')[0])
    assert q['total'] == p['total'] and (q['column'], q['gaps']) == (1, 1) and q['fields'][3]['table'] == 7 and q['fields'][0]['table'] == 0
    # without layers: the plan the existing tests pin
    r = parse(run(exe, 'rows=12,gates=50,fields=0x9,rpb=3,nx=3,ny=2')[0])
    assert (r['block_cells'], r['nz'], r['total']) == (6, 0, 4 * 6 * 32)
    # the 1 GiB limit counts every layer: 1023 x 1023 cells, one field, 64 layers fit (1022 MiB), a second field does not
    assert 64 * 1023 * 1023 * 16 <= 1 << 30 < 2 * 64 * 1023 * 1023 * 16
    big = 'fields=%s,nx=1023,ny=1023,nz=64'
    assert parse(run(exe, big % '0x1')[0])['total'] == 64 * 1023 * 1023 * 16
    assert 'at most 1 GiB' in run(exe, big % '0x3')[0] and 'at most 1 GiB' in run(exe, 'rows=2,rpb=1,' + big % '0x1')[0]
    assert CP.state_bytes(CP.Composite('ZH', np.arange(1024.0), np.arange(1024.0), z_edges=np.arange(65.0)), 1) == 64 * 1023 * 1023 * 16


def test_host_header_pass_keeps_layers_tables_and_gaps(exe):
    begin, more, end = COL + ',phase=1', COL + ',phase=0', COL + ',phase=2'
    out = run(exe, begin, more, more + ',ez=0:500:1001', more + ',ez=0:500:1000.00001', more + ',tf0=1:1.25', more + ',tv0=2:3.5',
              more + ',gaps=1', 'phase=0,nz=2', 'phase=0,products=65,nz=3,tab0=3', 'phase=0', 'phase=0,products=65,nz=2,tab0=4', end, more)
    assert parse(out[0])['open'] == 1 and parse(out[1])['open'] == 1
    assert 'height layers differ from the open pass' in out[2]
    assert parse(out[3])['open'] == 1                      # (the same edge after the rounding: the same pass)
    assert 'column table differs' in out[4] and 'column table differs' in out[5] and 'gaps differ' in out[6]
    assert 'products or block count differ' in out[7] and 'height layers differ' in out[8] and 'products or block count differ' in out[9]
    assert 'column table differs' in out[10]
    # the refusals left the pass as it was: it finishes, and is closed then
    assert parse(out[11])['open'] == 0 and 'no pass open' in out[12]
    # a plain pass takes no layers later, a layered pass no plain call
    out = run(exe, 'phase=1', 'phase=0,nz=1', 'phase=2', 'phase=1,nz=1', 'phase=0', 'phase=2,nz=1')
    assert 'height layers differ' in out[1] and parse(out[2])['open'] == 0 and 'height layers differ' in out[4] and parse(out[5])['open'] == 0
