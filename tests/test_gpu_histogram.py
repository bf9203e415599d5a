"""Sweep histograms on the GPU, the kernel alone (k_hist through cpol_debug_read "histogram_fields"): hand-built rows no sweep
produces, every count against histogram.count of the same rows.  The counts are integers and the bin of a value is found by
comparisons alone, so every comparison here is exact.

S = the gates a workgroup owns (histogram.STRETCH, checked against the library).  S = 512, so that a 360 x 500 sweep gives a
few hundred workgroups per field: no stretch holds more than 65 535 gates, and no LDS cell ever exceeds S.  The 16-bit case is
therefore more than 65 535 gates in ONE CELL of one block over ~200 stretches: a 16-bit counter in the uint64 state and a lost
flush both show there; a 16-bit LDS cell cannot show at any input and is not looked for."""
import functools

import numpy as np
import pytest

from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

F32 = np.float32
FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL']
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


def HG():
    from cosmo_pol_amd import histogram
    return histogram


def stretch():
    S = context().histogram_stretch()
    assert S == HG().STRETCH and 0 < S < 2 ** 32
    return S


def dtype_of(k):
    return np.float64 if k == 'RVEL' else F32


def field(rng, shape, k, edges=None):
    """Random values with gaps, infinities, signed zeros and -- where edges are given -- values on the edges and beside them."""
    dt = dtype_of(k)
    x = (rng.standard_normal(shape) * 3.0).astype(dt)
    flat = x.reshape(-1)
    if edges is not None and flat.size >= 8:
        e = np.asarray(edges, dtype=np.float64).astype(dt)
        pool = np.concatenate([e, np.nextafter(e, dt(-np.inf)), np.nextafter(e, dt(np.inf))])
        where = rng.random(flat.size) < 0.2
        flat[where] = rng.choice(pool, int(where.sum()))
    for value, share in ((np.nan, 0.15), (np.inf, 0.02), (-np.inf, 0.02), (-0.0, 0.02), (0.0, 0.02)):
        flat[rng.random(flat.size) < share] = value
    return x


def counting(pg, spec, k, n_blocks):
    """The counting gates of field k per block, from the definition: neither the value nor the ordinate NaN."""
    v = np.asarray(pg[k])
    v = v.reshape(-1, v.shape[-1])
    ok = v == v
    if spec.ordinate is not None:
        y = pg['model_vars'][spec.ordinate[1]] if isinstance(spec.ordinate, tuple) else pg[spec.ordinate]
        y = np.asarray(y).reshape(-1, v.shape[-1])
        ok &= (y == y)[np.arange(v.shape[0]) % y.shape[0]]
    return ok.reshape(n_blocks, -1).sum(axis=1)


def check(pg, spec, rpb=0, tag=''):
    got = context().histogram_fields(pg, spec, rpb)
    want = HG().count(pg, spec, rpb)
    assert sorted(got) == sorted(spec.fields), tag
    for k in spec.fields:
        assert got[k].dtype == np.uint64 and got[k].shape == want[k].shape, (tag, k, got[k].shape, want[k].shape)
        bad = int((got[k] != want[k]).sum())
        assert bad == 0, (tag, k, bad, int(got[k].sum()), int(want[k].sum()))
        nb = got[k].shape[0]
        assert np.array_equal(got[k].reshape(nb, -1).sum(axis=1), counting(pg, spec, k, nb)), (tag, k, 'sum')
    return got


EX = [-4.0, -1.0, -0.0, 0.5, 1.0, 2.5]
EY = [-2.0, 0.0, 0.1, 3.0]


def test_every_stretch_length_and_block_shape():
    H, S = HG(), stretch()
    rng = np.random.default_rng(5)
    specs = [H.Histogram({'ZH': EX}), H.Histogram({'KDP': EX, 'RVEL': EY}, ordinate='heights', ordinate_edges=EY)]
    n = 0
    for n_gates in (1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1):
        for n_rows in (1, 3):
            pg = {'ZH': field(rng, (n_rows, n_gates), 'ZH', EX), 'KDP': field(rng, (n_rows, n_gates), 'KDP', EX),
                  'RVEL': field(rng, (n_rows, n_gates), 'RVEL', EY), 'heights': field(rng, (n_rows, n_gates), 'ZH', EY)}
            for rpb in sorted({0, 1, n_rows}):
                for spec in specs:
                    check(pg, spec, rpb, 'gates %d rows %d rpb %d %r' % (n_gates, n_rows, rpb, spec))
                    n += 1
    assert n >= 100
    # a block border inside what would be one stretch: rows of S // 2 + 3 gates, one block per row and per two rows
    pg = {'ZH': field(rng, (4, S // 2 + 3), 'ZH', EX)}
    a = check(pg, specs[0], 1, 'border/1')['ZH']
    b = check(pg, specs[0], 2, 'border/2')['ZH']
    assert np.array_equal(a.reshape(2, 2, -1).sum(axis=1), b) and len({tuple(r) for r in a}) == 4


def test_smallest_and_largest_tables():
    H = HG()
    rng = np.random.default_rng(6)
    pg = {'ZH': field(rng, (3, 700), 'ZH', [0.0]), 'heights': field(rng, (3, 700), 'ZH', [0.0])}
    got = check(pg, H.Histogram({'ZH': [0.0, 1.0]}), 0, 'n_x = 1')['ZH']
    assert got.shape == (1, 3) and (got > 0).all()
    # exactly 16 384 cells (128 x 128): beyond 64 KiB of LDS with the edges beside the table
    e = np.linspace(-3.0, 3.0, 127)
    spec = H.Histogram({'ZH': e}, ordinate='heights', ordinate_edges=e)
    assert spec.cells == 16384
    got = check(pg, spec, 0, '16384 cells')['ZH']
    assert (got > 0).sum() > 500
    check(pg, spec, 1, '16384 cells per ray')
    # 16 385 = 145 x 113 cells is refused, by the specification and by the library
    with pytest.raises(ValueError):
        H.Histogram({'ZH': np.arange(144.0)}, ordinate='heights', ordinate_edges=np.arange(112.0))
    small = H.Histogram({'ZH': [0.0, 1.0]}, ordinate='heights', ordinate_edges=np.arange(112.0))
    wide = np.arange(144.0)

    def widen(h):
        h.n_x[0], h.edges_x[0] = 143, wide.ctypes.data
        return wide
    with pytest.raises(ValueError, match='16384'):
        context().histogram_fields(pg, small, tamper=widen)
    # 1023 bins on one axis: 1024 edges, the longest search; as abscissa (float32), as abscissa of RVEL and as ordinate (float64)
    e = np.linspace(-4.0, 4.0, 1024)
    pg['RVEL'] = field(rng, (3, 700), 'RVEL', e[::50])
    check(pg, H.Histogram({'ZH': e, 'RVEL': e}), 0, '1023 bins')
    check(pg, H.Histogram({'ZH': [0.0, 1.0]}, ordinate='RVEL', ordinate_edges=e), 0, '1023 ordinate bins')
    for n_edges in (2, 3, 4, 5, 7, 8, 9, 511, 512, 513, 1023):               # every first step of the search
        check(pg, H.Histogram({'ZH': np.linspace(-3.0, 3.0, n_edges)}), 0, '%d edges' % n_edges)


def test_every_gate_in_one_cell():
    H, S = HG(), stretch()
    n = 100003
    assert n > 65535 and n > 2 * S
    for k in ('ZH', 'RVEL'):
        pg = {k: np.full((1, n), 5.0, dtype=dtype_of(k)), 'heights': np.full((1, n), 2.0, dtype=F32)}
        got = check(pg, H.Histogram({k: [0.0, 4.0, 6.0]}), 0, 'one cell ' + k)[k]
        assert got.tolist() == [[0, 0, n, 0]]
        got = check(pg, H.Histogram({k: [0.0, 4.0, 6.0]}, ordinate='heights', ordinate_edges=[1.0, 3.0]), 0, 'one cell 2-D ' + k)[k]
        assert got[0, 1, 2] == n and got.sum() == n
    # ... and in two blocks of more than 65 535 gates each
    pg = {'ZH': np.full((2, 70001), 5.0, dtype=F32)}
    assert check(pg, H.Histogram({'ZH': [0.0, 4.0, 6.0]}), 1, 'one cell per block')['ZH'].tolist() == [[0, 0, 70001, 0]] * 2


def test_all_fields_types_and_ordinates():
    H = HG()
    rng = np.random.default_rng(7)
    n_rows, n_gates = 6, 333
    pg = {k: field(rng, (n_rows, n_gates), k, EX) for k in FIELDS}
    pg['heights'] = field(rng, (2, n_gates), 'ZH', EY)            # the geometry of an ensemble call: 2 rays, 3 members
    pg['dist'] = field(rng, (2, n_gates), 'ZH', EY)
    pg['model_vars'] = {'T': field(rng, (n_rows, n_gates), 'RVEL', EY), 'P': field(rng, (n_rows, n_gates), 'RVEL', EY)}
    every = {k: EX if i % 2 else EY for i, k in enumerate(FIELDS)}
    for ordinate in (None, 'heights', 'dist', 'RVEL', 'ZH', 'RHOHV', ('model', 'T'), ('model', 'P')):
        spec = H.Histogram(every, ordinate=ordinate, ordinate_edges=None if ordinate is None else EY)
        for rpb in (0, 2, 1):
            check(pg, spec, rpb, 'all fields / %r / %d' % (ordinate, rpb))
    for k, e in (('RVEL', EY), ('ZH', EX)):                     # a field as its own ordinate: the diagonal alone
        c = check(pg, H.Histogram({k: e}, ordinate=k, ordinate_edges=e), 0, 'own ordinate ' + k)[k][0]
        assert c.sum() == np.trace(c) > 0
    assert not np.array_equal(context().histogram_fields(pg, H.Histogram({'ZH': EX}, ('model', 'T'), EY))['ZH'],
                              context().histogram_fields(pg, H.Histogram({'ZH': EX}, ('model', 'P'), EY))['ZH'])


def test_value_classes():
    H = HG()
    nan, inf = np.nan, np.inf

    def one(k, values, edges, y=None, ey=None):
        pg = {k: np.array([values], dtype=dtype_of(k))}
        if y is not None:
            pg['dist'] = np.array([y], dtype=F32)
        spec = H.Histogram({k: edges}, ordinate=None if y is None else 'dist', ordinate_edges=ey)
        return check(pg, spec, 0, '%s %r' % (k, values))[k][0]
    for k in ('ZH', 'RVEL'):
        dt = dtype_of(k)
        assert one(k, [2.0], [1.0, 2.0, 4.0]).tolist() == [0, 0, 1, 0]
        assert one(k, [np.nextafter(dt(2.0), dt(0))], [1.0, 2.0, 4.0]).tolist() == [0, 1, 0, 0]
        assert one(k, [np.nextafter(dt(2.0), dt(9))], [1.0, 2.0, 4.0]).tolist() == [0, 0, 1, 0]
        assert one(k, [4.0, np.nextafter(dt(4.0), dt(0)), 1.0, np.nextafter(dt(1.0), dt(0))], [1.0, 2.0, 4.0]).tolist() == [1, 1, 1, 1]
        assert one(k, [-0.0, 0.0], [-1.0, 0.0, 1.0]).tolist() == [0, 0, 2, 0]
        assert one(k, [-0.0, 0.0], [-1.0, -0.0, 1.0]).tolist() == [0, 0, 2, 0]
        assert one(k, [inf, -inf, nan], [-1.0, 0.0, 1.0]).tolist() == [1, 0, 0, 1]
        got = one(k, [1.5, nan, 1.5, nan, 0.5], [1.0, 2.0], y=[10.0, 10.0, nan, nan, -5.0], ey=[0.0, 20.0])
        want = np.zeros((3, 3), dtype=np.uint64)
        want[1, 1] = want[0, 0] = 1
        assert np.array_equal(got, want)
    # the edge is the rounded one: float32(0.1) sits on it, its lower neighbour below
    assert one('ZH', [F32(0.1), np.nextafter(F32(0.1), F32(0))], [0.1, 1.0]).tolist() == [1, 1, 0]
    assert one('RVEL', [0.1, float(F32(0.1))], [0.1, 1.0]).tolist() == [0, 2, 0]


def test_pass_mechanics():
    H = HG()
    ctx = context()
    rng = np.random.default_rng(8)
    spec = H.Histogram({'ZH': EX, 'RVEL': EY}, ordinate='heights', ordinate_edges=EY)
    pg = {'ZH': field(rng, (3, 600), 'ZH', EX), 'RVEL': field(rng, (3, 600), 'RVEL', EY), 'heights': field(rng, (3, 600), 'ZH', EY)}
    part = lambda a, b: {k: v[a:b] for k, v in pg.items()}                      # noqa: E731
    whole = check(pg, spec, 0, 'one call of 3')
    # 1 + 2 against 3
    assert ctx.histogram_fields(part(0, 1), spec, phase=1) is None
    got = ctx.histogram_fields(part(1, 3), spec, phase=2)
    assert all(np.array_equal(got[k], whole[k]) for k in spec.fields)
    # a second pass right behind it: the begin clears
    assert ctx.histogram_fields(part(0, 2), spec, phase=1) is None
    assert ctx.histogram_fields(part(2, 3), spec, phase=0) is None
    got = ctx.histogram_fields(part(0, 1), spec, phase=2)
    want = H.count(part(0, 1), spec, into=H.count(pg, spec))
    assert all(np.array_equal(got[k], want[k]) for k in spec.fields)
    # a begin in the middle of an open pass starts over
    ctx.histogram_fields(pg, spec, phase=1)
    ctx.histogram_fields(part(0, 1), spec, phase=1)
    got = ctx.histogram_fields(part(1, 2), spec, phase=2)
    assert all(np.array_equal(got[k], H.count(part(0, 2), spec)[k]) for k in spec.fields)
    # calls of other shapes fold into a pass of one block
    other = {'ZH': field(rng, (2, 77), 'ZH', EX), 'RVEL': field(rng, (2, 77), 'RVEL', EY), 'heights': field(rng, (1, 77), 'ZH', EY)}
    ctx.histogram_fields(pg, spec, phase=1)
    got = ctx.histogram_fields(other, spec, phase=2)
    want = H.count(other, spec, into=H.count(pg, spec))
    assert all(np.array_equal(got[k], want[k]) for k in spec.fields)
    # refused calls in the middle leave the state untouched: the pass finishes as if they had not been made
    ctx.histogram_fields(part(0, 1), spec, phase=1)
    with pytest.raises(ValueError, match='differ'):
        ctx.histogram_fields(part(1, 3), H.Histogram({'ZH': EX}, ordinate='heights', ordinate_edges=EY), phase=0)
    with pytest.raises(ValueError, match='differ'):
        ctx.histogram_fields(part(1, 3), H.Histogram({'ZH': EX, 'RVEL': EY}, ordinate='heights', ordinate_edges=EY[:-1] + [9.0]), phase=0)
    with pytest.raises(ValueError, match='differ'):
        ctx.histogram_fields(part(1, 3), spec, rays_per_block=1, phase=0)
    with pytest.raises(ValueError, match='phase'):
        ctx.histogram_fields(part(1, 3), spec, phase=5)
    got = ctx.histogram_fields(part(1, 3), spec, phase=2)
    assert all(np.array_equal(got[k], whole[k]) for k in spec.fields)
    # the pass is closed now
    with pytest.raises(ValueError, match='no pass open'):
        ctx.histogram_fields(pg, spec, phase=0)
    with pytest.raises(ValueError, match='no pass open'):
        ctx.histogram_fields(pg, spec, phase=2)
    # with blocks: every call gives the same number of them
    ctx.histogram_fields(part(0, 2), spec, rays_per_block=1, phase=1)
    with pytest.raises(ValueError, match='differ'):
        ctx.histogram_fields(pg, spec, rays_per_block=1, phase=0)
    got = ctx.histogram_fields(part(1, 3), spec, rays_per_block=1, phase=2)
    want = H.count(part(1, 3), spec, 1, into=H.count(part(0, 2), spec, 1))
    assert all(np.array_equal(got[k], want[k]) for k in spec.fields)


def test_refusals_leave_the_context_usable():
    H = HG()
    ctx = context()
    rng = np.random.default_rng(9)
    pg = {'ZH': field(rng, (4, 90), 'ZH', EX), 'RVEL': field(rng, (4, 90), 'RVEL', EY), 'heights': field(rng, (4, 90), 'ZH', EY),
          'model_vars': {'T': field(rng, (4, 90), 'RVEL', EY)}}
    spec = H.Histogram({'ZH': EX, 'RVEL': EY}, ordinate='heights', ordinate_edges=EY)
    flat = H.Histogram({'ZH': EX})
    good = check(pg, spec, 2, 'before')
    bad_edges = {'nan': np.array([0.0, np.nan, 2.0]), 'inf': np.array([0.0, 1.0, np.inf]), 'desc': np.array([0.0, 2.0, 1.0]),
                 'equal': np.array([0.0, 1.0, 1.0]), 'collapse': np.array([0.0, 1.0, 1.0 + 1e-9]), 'huge': np.array([0.0, 1.0, 1e39])}

    def setter(**kw):
        def change(h):
            for k, v in kw.items():
                setattr(h, k, v)
        return change

    def edges_x(k, name):
        def change(h):
            h.n_x[k], h.edges_x[k] = len(bad_edges[name]) - 1, bad_edges[name].ctypes.data
        return change

    def edges_y(name):
        def change(h):
            h.n_y, h.edges_y = len(bad_edges[name]) - 1, bad_edges[name].ctypes.data
        return change

    def index(name, k, v):
        def change(h):
            getattr(h, name)[k] = v
        return change
    bad = [setter(phase=4), setter(phase=-1), setter(fields=0), setter(fields=1 << 10), setter(fields=0x401),
           setter(ordinate=3), setter(ordinate=15), setter(ordinate=26), setter(ordinate=31), setter(ordinate=56), setter(ordinate=-1),
           setter(ordinate=33),                                   # v >= n_vars (one model variable given)
           setter(n_y=0), setter(n_y=-2), setter(edges_y=None), setter(n_y=1024),
           setter(ordinate=0),                                    # n_y != 0 with ordinate 0
           index('n_x', 0, 0), index('n_x', 0, -1), index('n_x', 0, 1024), index('n_x', 9, 0), index('edges_x', 0, None),
           index('edges_x', 9, None), index('counts', 0, None), index('counts', 9, None),
           setter(rays_per_block=-1), setter(rays_per_block=3), setter(rays_per_block=8)]
    bad += [edges_x(0, n) for n in bad_edges] + [edges_x(9, n) for n in bad_edges if n not in ('collapse', 'huge')]
    bad += [edges_y(n) for n in bad_edges]
    for i, change in enumerate(bad):
        with pytest.raises(ValueError):
            ctx.histogram_fields(pg, spec, 2, tamper=change)
        if i % 8 == 0:
            got = ctx.histogram_fields(pg, spec, 2)
            assert all(np.array_equal(got[k], good[k]) for k in spec.fields), i
    # float64 keeps what float32 collapses: RVEL takes those edges
    ctx.histogram_fields(pg, spec, 2, tamper=edges_x(9, 'collapse'))
    ctx.histogram_fields(pg, spec, 2, tamper=edges_x(9, 'huge'))
    # an ordinate 32 + v when the call has no model_vars; a requested field or an ordinate without its input
    no_model = {k: v for k, v in pg.items() if k != 'model_vars'}
    with pytest.raises(ValueError, match='model'):
        ctx.histogram_fields(no_model, flat, tamper=lambda h: (setattr(h, 'ordinate', 32), setattr(h, 'n_y', 1), setattr(
            h, 'edges_y', bad_edges['desc'].ctypes.data)))
    with pytest.raises(ValueError, match='no input'):
        ctx.histogram_fields({'ZH': pg['ZH']}, flat, phase=1, tamper=setter(fields=0b11, n_x=flat_nx(2), edges_x=flat_ex(bad_edges)))
    with pytest.raises(ValueError, match='no input'):
        ctx.histogram_fields({'ZH': pg['ZH']}, H.Histogram({'ZH': EX}, ordinate='heights', ordinate_edges=EY))
    # the three limits
    with pytest.raises(ValueError, match='2\\^27'):
        e = np.linspace(-3.0, 3.0, 127)
        big = {'ZH': np.zeros((8192, 1), dtype=F32), 'ZV': np.zeros((8192, 1), dtype=F32), 'heights': np.zeros((8192, 1), dtype=F32)}
        ctx.histogram_fields(big, H.Histogram({'ZH': e, 'ZV': [0.0, 1.0]}, ordinate='heights', ordinate_edges=e), 1, phase=1)
    # nothing was queued, the context is usable: the same call, the same counts
    got = ctx.histogram_fields(pg, spec, 2)
    assert all(np.array_equal(got[k], good[k]) for k in spec.fields)
    check(pg, H.Histogram({'ZH': EX}, ordinate=('model', 'T'), ordinate_edges=EY), 0, 'after the refusals')


def flat_nx(n):
    import ctypes as C
    a = (C.c_int32 * 10)()
    a[0] = a[1] = n
    return a


def flat_ex(keep):
    import ctypes as C
    keep['two'] = np.array([0.0, 1.0, 2.0])
    a = (C.c_void_p * 10)()
    a[0] = a[1] = keep['two'].ctypes.data
    return a
