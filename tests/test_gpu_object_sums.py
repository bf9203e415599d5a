"""The exact sums of the object cells on the GPU, the kernels alone (k_obj_sums and k_obj_sums_finish behind k_obj_decode through
cpol_debug_read "fractions_maps"): hand-built maps no sweep produces against objects.cells of the same maps.  Every sum is a sum
of integers rounded once, so every comparison is on the bits (view(uint64) equality): no tolerance anywhere.  In each case the
RULE is asserted first to find an object with a non-zero volume, so that an idle kernel cannot pass.  The integer attributes, the
labels and the scores of the same call are compared with the call without sums: the sums change nothing of them."""
import numpy as np
import pytest

from _objects import PATTERNS, SHAPES, pattern
from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

f4, f8, u1, u4, u8, i4 = np.float32, np.float64, np.uint8, np.uint32, np.uint64, np.int32
inf, nan = np.inf, np.nan
FLT_MAX = np.finfo(f4).max
INTS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')
FLOATS = ('volume', 'moment_x', 'moment_y')
SCORES = ('diff2', 'forecast2', 'observed2', 'n_forecast', 'n_observed', 'n_domain')
ONE, FOUR = [0.75], [-inf, 0.0, 3.0, inf]
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


def OB():
    from cosmo_pol_amd import objects
    return objects


def spec_for(n_y, n_x, thresholds, **kw):
    from cosmo_pol_amd import composite, neighbourhood
    kw.setdefault('sums', True)
    return OB().Objects(neighbourhood.Fractions(composite.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0)), 'ZH', thresholds, [0]), **kw)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: u4, 8: u8}[a.dtype.itemsize])


def same_side(got, want, tag):
    for k in INTS + ('skipped',):
        assert got[k].dtype == u4 and np.array_equal(got[k], want[k]), (tag, k, got[k].ravel()[:8], want[k].ravel()[:8])
    assert np.array_equal(bits(got['peak']), bits(want['peak'])), (tag, 'peak')
    if 'labels' in want:
        assert np.array_equal(got['labels'], want['labels']), (tag, 'labels')
    for k in FLOATS:
        assert got[k].dtype == f8 and got[k].shape == want[k].shape, (tag, k)
        bad = bits(got[k]) != bits(want[k])
        assert not bad.any(), (tag, k, int(bad.sum()), got[k][bad][:4], want[k][bad][:4])
        assert np.array_equal(bits(got['field'][k]), bits(want['field'][k])), (tag, 'field', k, got['field'][k], want['field'][k])
    for k in ('cells', 'skipped'):
        assert np.asarray(got['field'][k]).dtype == u4 and np.array_equal(got['field'][k], want['field'][k]), (tag, 'field', k)


def check(maps, obs, thresholds, domain=None, tag='', skipped=False, **kw):
    maps = maps if maps.ndim == 3 else maps[None]
    spec = spec_for(obs.shape[0], obs.shape[1], thresholds, **kw)
    want = OB().cells(spec, maps, obs, domain)
    # the rule itself: an object with a non-zero volume, and a field that sums something
    assert (want['volume'] != 0).any() or (want['observed']['volume'] != 0).any(), (tag, 'the rule finds no object with a volume')
    assert int(want['field']['cells'].sum()) + int(want['observed']['field']['cells']) > 0, (tag, 'the rule sums no cell')
    if skipped:
        assert int(want['skipped'].sum()) > 0 and int(want['field']['skipped'].sum()) > 0, (tag, 'the rule skips no cell')
    ctx = context()
    scores, got = ctx.fractions_maps(maps, obs, spec.fractions, domain=domain, objects=spec)
    same_side(got, want, tag)
    same_side(got['observed'], want['observed'], (tag, 'observed'))
    assert got['grid'] == want['grid'] and (got['weight'] is None) == (want['weight'] is None)
    # the same call once more: the same bits; and without the sums: the same cells and scores, and no new key
    scores2, again = ctx.fractions_maps(maps, obs, spec.fractions, domain=domain, objects=spec)
    for side_a, side_b in ((again, got), (again['observed'], got['observed'])):
        for k in FLOATS:
            assert np.array_equal(bits(side_a[k]), bits(side_b[k])) and np.array_equal(bits(side_a['field'][k]), bits(side_b['field'][k])), (tag, 'twice', k)
    off = spec_for(obs.shape[0], obs.shape[1], thresholds, **dict(kw, sums=False, weight=None))
    scores0, plain = ctx.fractions_maps(maps, obs, off.fractions, domain=domain, objects=off)
    assert not {'volume', 'moment_x', 'moment_y', 'skipped', 'field', 'weight', 'grid'} & (set(plain) | set(plain['observed'])), tag
    for side_a, side_b in ((plain, got), (plain['observed'], got['observed'])):
        for k in INTS + (('labels',) if off.labels else ()):
            assert np.array_equal(side_a[k], side_b[k]), (tag, 'sums off', k)
        assert np.array_equal(bits(side_a['peak']), bits(side_b['peak'])), (tag, 'sums off', 'peak')
    for k in SCORES:
        assert np.array_equal(scores[k], scores0[k]) and np.array_equal(scores[k], scores2[k]), (tag, k)
    return want


def wide(rng, shape, negatives=True):
    """float32 values whose exponents are drawn from the whole range: finite bit patterns, denormals among them."""
    raw = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(u4)
    raw = np.where(((raw >> u4(23)) & u4(0xFF)) == 0xFF, raw & u4(0x807FFFFF), raw)         # (an all-ones exponent becomes a denormal)
    if not negatives:
        raw = raw & u4(0x7FFFFFFF)
    return raw.view(f4)


def sprinkle(rng, v, pool, share=0.08):
    """Some cells of v replaced by members of `pool`."""
    v = v.copy()
    at = rng.random(v.shape) < share
    v[at] = np.array(pool, f4)[rng.integers(0, len(pool), int(at.sum()))]
    return v


SPECIAL = [FLT_MAX, -FLT_MAX, 0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 3.0]


def test_one_cell():
    want = check(np.full((1, 1), 2.5, f4), np.full((1, 1), nan, f4), ONE, tag='set against unset')
    assert want['volume'].tolist() == [[[2.5] + [0.0] * 1023]] and want['field']['cells'].tolist() == [1] and want['observed']['field']['cells'] == 0
    check(np.full((1, 1), nan, f4), np.full((1, 1), -FLT_MAX, f4), [-inf], tag='unset against a negative cell')
    check(np.full((1, 1), inf, f4), np.full((1, 1), 1e-45, f4), ONE + [0.0], skipped=True, max_objects=1, tag='an infinite cell against a denormal')


@pytest.mark.parametrize('n_y, n_x', [(1, 65), (3, 130), (67, 5)])
def test_whole_exponent_range_in_one_object(n_y, n_x):
    """Chunk borders, runs that cross them, more rows than a workgroup's four: every cell set (threshold -inf), so ONE object holds
    exponents from the denormals to FLT_MAX of both signs."""
    rng = np.random.default_rng(31 * n_y + n_x)
    maps = np.stack([sprinkle(rng, wide(rng, (n_y, n_x)), SPECIAL) for _ in range(2)])
    obs = sprinkle(rng, wide(rng, (n_y, n_x)), SPECIAL)
    want = check(maps, obs, [-inf], max_objects=3, tag='wide')
    assert want['n_objects'].tolist() == [[1], [1]] and want['area'][0, 0, 0] == n_y * n_x
    # NaN and +inf cells and a domain mask: objects fall apart, cells are skipped
    maps = sprinkle(rng, maps, [nan, inf, -inf], 0.1)
    maps[0, 0, 0] = inf
    dom = (rng.random((n_y, n_x)) < 0.8).astype(u1)
    dom[0, 0] = 1
    for connectivity in (4, 8):
        check(maps, sprinkle(rng, obs, [nan, inf], 0.1), [-inf, 0.0], domain=dom, connectivity=connectivity, skipped=True, max_objects=6, tag=('holes', connectivity))


def test_cancelling_triples_in_different_rows():
    """2^100, 1, -2^100 in three rows of one object: a sum that depends on the order loses the ones."""
    m = np.ones((7, 70), f4)
    m[0, 3], m[5, 66] = 2.0 ** 100, -2.0 ** 100
    m[1, 64], m[6, 1] = FLT_MAX, -FLT_MAX
    o = np.ones((7, 70), f4)
    o[2, 2], o[3, 69], o[4, 0] = -2.0 ** 100, 2.0 ** 100, 1e-45
    want = check(m, o, [-inf], tag='cancelling')
    assert want['volume'][0, 0, 0] == 7 * 70 - 4 and want['observed']['volume'][0, 0] == 7 * 70 - 3 + 1e-45
    assert want['field']['volume'][0] == 7 * 70 - 4
    assert want['moment_x'][0, 0, 0] == 7 * 70 * 69 / 2 - (3 + 66 + 64 + 1) + (3 - 66) * 2.0 ** 100 + float(FLT_MAX) * 63


@pytest.mark.parametrize('n_y, n_x', SHAPES)
@pytest.mark.parametrize('connectivity', [4, 8])
def test_patterns_equal_the_rule(n_y, n_x, connectivity):
    rng = np.random.default_rng(100 * n_y + n_x)

    def field(binary):
        hi = np.ldexp(1.0 + rng.random(binary.shape), rng.integers(0, 127, binary.shape)).astype(f4)
        return np.where(binary, hi, f4(-1.0)).astype(f4)
    maps = np.stack([field(pattern(name, (n_y, n_x))) for name in PATTERNS])
    for k in range(0, len(PATTERNS), 3):                  # three blocks and the observation in one call
        for min_area, max_objects in ((1, 4096), (2, 5))[:2 if n_y * n_x > 1 else 1]:      # (one cell: no object of two cells)
            check(maps[k:k + 3], maps[(k + 3) % len(PATTERNS)], ONE, connectivity=connectivity, min_area=min_area, max_objects=max_objects,
                  tag=(PATTERNS[k:k + 3], min_area))
    # max_objects below the number of objects: the rows of the table alone are summed
    board = field(pattern('checkerboard', (n_y, n_x)))
    want = check(board, board, ONE, connectivity=4, max_objects=2, labels=False, tag='overflow')
    assert int(want['n_objects'][0, 0]) == (n_y * n_x + 1) // 2 and (n_y * n_x < 4 or int(want['n_objects'][0, 0]) > 2)


def test_three_blocks_four_thresholds_and_a_domain():
    rng = np.random.default_rng(41)
    pool = SPECIAL + [nan, inf, -inf, 2.5, 3.0, 7.0, 2.0 ** 100, -2.0 ** 100, 1e-30]
    maps = np.array(pool, f4)[rng.integers(0, len(pool), (3, 33, 70))]
    maps[1] = sprinkle(rng, wide(rng, (33, 70)), pool, 0.3)
    obs = sprinkle(rng, wide(rng, (33, 70)), pool, 0.3)
    dom = (rng.random((33, 70)) < 0.7).astype(u1)
    for connectivity in (4, 8):
        want = check(maps, obs, FOUR, connectivity=connectivity, skipped=True, max_objects=64, tag=('pool', connectivity))
        assert (want['volume'][:, 0] < 0).any() and (want['volume'][:, 3] == 0).all() and want['skipped'][:, 3].any()      # (-inf sets negatives; +inf: skipped cells alone)
        check(maps, obs, FOUR, domain=dom, connectivity=connectivity, min_area=3, skipped=True, max_objects=16, tag=('pool, domain', connectivity))


def test_under_a_weight_table():
    """Values below, on and above the breakpoints, between them, next to them; a table whose last value overflows float32."""
    rng = np.random.default_rng(42)
    for tv, tf in (OB().zr_table(), OB().zr_table(300.0, 1.4, 5.0, 55.0, 0.5),
                   (np.array([-3.0, 0.0, 0.5, 7.0, 9.0], f4), np.array([-2.0, -1.0, -1.0, 4.0, 1e300]))):
        between = (tv[:-1].astype(f8) + rng.random(tv.size - 1) * (tv[1:].astype(f8) - tv[:-1])).astype(f4)
        v = np.concatenate([tv, between, np.nextafter(tv, f4(-inf)), np.nextafter(tv, f4(inf)),
                            np.array([tv[0] - 1, -inf, inf, tv[-1] * 2 + 1, -0.0, 0.0, 1e-42, FLT_MAX, -FLT_MAX, nan], f4)]).astype(f4)
        n_x = 67
        cells = np.resize(v, (-(-v.size // n_x) + 1) * n_x)
        maps = np.stack([cells.reshape(-1, n_x), rng.permutation(cells).reshape(-1, n_x)]).astype(f4)
        hot = tf[-1] > 1e38
        want = check(maps, rng.permutation(cells).reshape(-1, n_x), [-inf, float(tv[2])], weight=(tv, tf), skipped=hot, max_objects=8, connectivity=8,
                     tag=('table', tv.size))
        assert want['weight'] is not None and (want['volume'] > 0).any()


def test_the_bound_case():
    """1023 x 1023 cells of FLT_MAX in one object: the bins at their bounds."""
    full = np.full((1023, 1023), FLT_MAX, f4)
    want = check(full, np.zeros((1023, 1023), f4), [1.0], max_objects=2, labels=False, tag='bound')
    M = ((1 << 24) - 1) << 254
    assert want['n_objects'].tolist() == [[1]] and want['area'][0, 0, 0] == 1023 * 1023
    assert bits(want['volume'][0, 0, :1])[0] == bits(np.array([OB().round_scaled(M * 1023 * 1023)]))[0]
    assert bits(want['moment_x'][0, 0, :1])[0] == bits(np.array([OB().round_scaled(M * 1023 * (1022 * 1023 // 2))]))[0]
    assert want['field']['cells'].tolist() == [1023 * 1023] and want['observed']['field']['volume'] == 0.0


def test_refusals_leave_the_context_usable():
    rng = np.random.default_rng(43)
    maps, obs = wide(rng, (2, 9, 70)), wide(rng, (9, 70))
    spec = spec_for(9, 70, [-inf], weight=OB().zr_table())
    ctx = context()

    def set_to(name, value):
        def tamper(f):
            o = f.objects.contents
            if value == 'misaligned':
                setattr(o, name, getattr(o, name) + 4)
            elif value == 'decreasing':
                tf = spec.weight[1].copy()
                tf[5] = tf[3]
                o.weight_f = tf.ctypes.data
                return tf
            elif value == 'flat':
                tv = spec.weight[0].copy()
                tv[7] = tv[6]
                o.weight_v = tv.ctypes.data
                return tv
            else:
                setattr(o, name, value)
        return tamper
    for name, value, what in (('sums', 2, 'sums must be 0 or 1'), ('sums', -1, 'sums must be 0 or 1'),
                              ('volume', None, 'volume, skipped, field or field_cells is NULL'), ('skipped', None, 'volume, skipped, field or field_cells is NULL'),
                              ('field', None, 'volume, skipped, field or field_cells is NULL'), ('field_cells', None, 'volume, skipped, field or field_cells is NULL'),
                              ('volume', 'misaligned', 'volume and field must be 8-byte aligned'), ('field', 'misaligned', 'volume and field must be 8-byte aligned'),
                              ('n_weight', 1, 'a weight table needs 2 ... 1024 breakpoints'), ('n_weight', 1025, 'a weight table needs 2 ... 1024 breakpoints'),
                              ('weight_v', None, 'weight_v or weight_f is NULL'), ('weight_f', None, 'weight_v or weight_f is NULL'),
                              ('weight_f', 'decreasing', 'the values of the weight table decrease'),
                              ('weight_v', 'flat', 'the breakpoints of the weight table are not strictly ascending')):
        with pytest.raises(ValueError, match='cpol_objects: ' + what):
            ctx.fractions_maps(maps, obs, spec.fractions, objects=spec, tamper=set_to(name, value))
    check(maps, obs, [-inf], weight=OB().zr_table(), tag='after the refusals')
    # the labelling scratch of 32 sources x 4 thresholds of 1023 x 1023 passes, the accumulators of 32 rows behind it do not (refused
    # before anything is uploaded: the maps are pages never touched)
    big = spec_for(1023, 1023, FOUR, max_objects=32, labels=False)
    assert OB().scratch_bytes(big, 31) > OB().MAX_SCRATCH_BYTES >= OB().scratch_bytes(spec_for(1023, 1023, FOUR, max_objects=32, sums=False), 31)
    with pytest.raises(ValueError, match='cpol_objects: the labelling scratch and the sums'):
        ctx.fractions_maps(np.zeros((31, 1023, 1023), f4), np.zeros((1023, 1023), f4), big.fractions, objects=big)
    check(maps, obs, [-inf], tag='after the refused scratch')
