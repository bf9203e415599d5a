"""The match of the object cells on the GPU, the kernels alone (k_match_runs, the objects' kernels on the piece arrays, k_match_attr
and k_match_decode behind everything else through cpol_debug_read "fractions_maps"): hand-built maps no sweep produces against
objects.cells of the same maps.  Every number is a count, an integer sum, an integer extreme or a comparison, so every comparison
is np.array_equal: no tolerance anywhere.  In each case the RULE is asserted first to find at least one piece, and in the
multi-piece cases more pieces than (forecast, observed) pairs, so that an idle kernel cannot pass.  The cells, the exact sums and
the scores of the same call are compared too, and with the call without the match: the match changes nothing of them."""
import ctypes as C

import numpy as np
import pytest

from _objects import PATTERNS, SHAPES, pattern
from test_gpu_composite import values
from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

f4, u1, u4, u8, i4, i8 = np.float32, np.uint8, np.uint32, np.uint64, np.int32, np.int64
inf, nan = np.inf, np.nan
CELLS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')
PIECES = ('n_pieces', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'forecast', 'observed')
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


def mods():
    from cosmo_pol_amd import neighbourhood, objects
    return neighbourhood, objects


def spec_for(n_y, n_x, thresholds, **kw):
    from cosmo_pol_amd import composite
    NB, OB = mods()
    kw.setdefault('match', True)
    return OB.Objects(NB.Fractions(composite.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0)), 'ZH', thresholds, [0]), **kw)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: u4, 8: u8}[a.dtype.itemsize])


def same_cells(got, want, tag):
    """The cells, the labels and the exact sums of one side."""
    for k in CELLS + (('skipped',) if 'skipped' in want else ()):
        assert got[k].dtype == u4 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (tag, k, got[k].ravel()[:8], want[k].ravel()[:8])
    assert np.array_equal(bits(got['peak']), bits(want['peak'])), (tag, 'peak')
    assert ('labels' in got) == ('labels' in want) and ('volume' in got) == ('volume' in want), tag
    if 'labels' in want:
        assert got['labels'].dtype == i4 and np.array_equal(got['labels'], want['labels']), (tag, 'labels')
    if 'volume' in want:
        for k in FLOATS:
            assert np.array_equal(bits(got[k]), bits(want[k])) and np.array_equal(bits(got['field'][k]), bits(want['field'][k])), (tag, k)
        for k in ('cells', 'skipped'):
            assert np.array_equal(got['field'][k], want['field'][k]), (tag, 'field', k)


def same_match(got, want, tag):
    assert sorted(got['pieces']) == sorted(PIECES), tag
    for k in PIECES:
        g, w = got['pieces'][k], want['pieces'][k]
        assert g.dtype == u4 and g.shape == w.shape, (tag, k, g.shape, w.shape)
        assert np.array_equal(g, w), (tag, 'pieces', k, int((g != w).sum()), g.ravel()[:8], w.ravel()[:8])
    for k in ('covered', 'covered_observed'):
        assert got[k].dtype == u4 and got[k].shape == want[k].shape, (tag, k)
        assert np.array_equal(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()), got[k].ravel()[:8], want[k].ravel()[:8])


def pairs_of(labels, observed_labels):
    """int64 [n_blocks]: the distinct (forecast, observed) pairs of every block, summed over the thresholds, counted from the cells."""
    n = np.zeros(labels.shape[0], i8)
    for b in range(labels.shape[0]):
        for t in range(labels.shape[1]):
            both = (labels[b, t] > 0) & (observed_labels[t] > 0)
            n[b] += np.unique(labels[b, t][both].astype(i8) * (1 << 20) + observed_labels[t][both]).size
    return n


def check(maps, obs, thresholds, domain=None, multi=False, busy=True, tag='', **kw):
    NB, OB = mods()
    maps = maps if maps.ndim == 3 else maps[None]
    spec = spec_for(obs.shape[0], obs.shape[1], thresholds, **kw)
    want = OB.cells(spec, maps, obs, domain)
    found = int(want['pieces']['n_pieces'].sum(dtype=i8))
    assert found > 0 or not busy, (tag, 'the rule itself finds no piece')
    if multi:
        full = want if spec.labels else OB.cells(spec_for(obs.shape[0], obs.shape[1], thresholds, **dict(kw, labels=True)), maps, obs, domain)
        n_pairs = int(pairs_of(full['labels'], full['observed']['labels']).sum())
        assert found > n_pairs, (tag, 'no pair in more than one piece', found, n_pairs)
    ctx = context()
    scores, got = ctx.fractions_maps(maps, obs, spec.fractions, domain=domain, objects=spec)
    same_match(got, want, tag)
    same_cells(got, want, tag)
    same_cells(got['observed'], want['observed'], (tag, 'observed'))
    want_scores = NB.sums(spec.fractions, maps, obs, domain)
    for k in SCORES:
        assert np.array_equal(scores[k], want_scores[k]), (tag, k)
    # the invariants on the device result, where nothing overflows
    pc = got['pieces']
    n_max = max(int(got['n_objects'].max()), int(got['observed']['n_objects'].max()))
    if int(pc['n_pieces'].max()) <= spec.max_pieces and n_max <= spec.max_objects:
        cells = pc['area'].sum(axis=-1, dtype=u8)
        assert np.array_equal(cells, got['covered'].sum(axis=-1, dtype=u8)) and np.array_equal(cells, got['covered_observed'].sum(axis=-1, dtype=u8)), tag
        assert (got['covered'] <= got['area']).all() and (got['covered_observed'] <= got['observed']['area'][None]).all(), tag
        if 'labels' in got:
            both = (got['labels'] > 0) & (got['observed']['labels'] > 0)[None]
            assert np.array_equal(cells, both.sum(axis=(-2, -1), dtype=u8)), (tag, 'the cells of the overlap map')
    # the same call without the match: every output equals today's, and no new key
    off = spec_for(obs.shape[0], obs.shape[1], thresholds, **dict(kw, match=False, max_pieces=None))
    scores0, plain = ctx.fractions_maps(maps, obs, off.fractions, domain=domain, objects=off)
    assert not {'pieces', 'covered', 'covered_observed'} & set(plain) and set(plain) | {'pieces', 'covered', 'covered_observed'} == set(got), tag
    same_cells(plain, got, (tag, 'match off'))
    same_cells(plain['observed'], got['observed'], (tag, 'match off, observed'))
    for k in SCORES:
        assert np.array_equal(scores[k], scores0[k]), (tag, 'match off', k)
    return want


def field(binary, rng=None):
    """float32 values whose cells >= 0.75 are those of `binary`."""
    hi = np.full(binary.shape, 5.0, f4) if rng is None else (1.0 + rng.integers(0, 50, binary.shape)).astype(f4)
    return np.where(binary, hi, f4(-1.0)).astype(f4)


def test_one_cell():
    one = np.full((1, 1), 2.0, f4)
    for connectivity in (4, 8):
        want = check(one, one, ONE, connectivity=connectivity, tag='one cell')
        assert want['pieces']['n_pieces'].tolist() == [[1]] and want['covered'].shape == (1, 1, 1024)
        assert (want['pieces']['forecast'][0, 0, 0], want['pieces']['observed'][0, 0, 0], want['covered'][0, 0, 0]) == (1, 1, 1)


@pytest.mark.parametrize('n_y, n_x', SHAPES)
@pytest.mark.parametrize('connectivity', [4, 8])
def test_pattern_pairs_equal_the_rule(n_y, n_x, connectivity):
    """Three blocks and an observation per call, cycling through all 64 pairs of the patterns.  A single pair may share no cell
    ('run' is empty on a grid one cell wide), so the case as a whole asserts that the rule finds pieces, and at 65 x 67 that it finds
    more pieces than pairs for as many of the 64 pairs as the rule was found to give on the CPU: 30 under 8-connectivity, 10 under 4."""
    rng = np.random.default_rng(100 * n_y + n_x)
    maps = np.stack([field(pattern(name, (n_y, n_x)), rng) for name in PATTERNS])
    n = len(PATTERNS)
    pieces, split = 0, set()
    for o in range(n):
        for blocks in ([0, 1, 2], [3, 4, 5], [6, 7, o]):
            want = check(maps[blocks], maps[o], ONE, connectivity=connectivity, busy=False, max_objects=4096, max_pieces=4096,
                         tag=([PATTERNS[b] for b in blocks], PATTERNS[o]))
            pieces += int(want['pieces']['n_pieces'].sum())
            more = want['pieces']['n_pieces'][:, 0] > pairs_of(want['labels'], want['observed']['labels'])
            split |= {(b, o) for b, m in zip(blocks, more) if m}
    assert pieces > 0, 'the rule itself finds no piece'
    if (n_y, n_x) == (65, 67):
        assert len(split) == {4: 10, 8: 30}[connectivity], sorted(split)


def test_checkerboard_against_full():
    board, full = pattern('checkerboard', (65, 67)), pattern('full', (65, 67))
    want = check(np.stack([field(board), field(full)]), field(full), ONE, connectivity=4, max_objects=4096, max_pieces=4096, tag='board')
    assert want['pieces']['n_pieces'].ravel().tolist() == [2178, 1] and (want['pieces']['area'][0, 0, :2178] == 1).all()
    assert want['pieces']['forecast'][0, 0, 2177] == 2178 and want['covered_observed'][0, 0, 0] == 2178 and want['covered'][1, 0, 0] == 65 * 67
    # the other way round the observed side has the single cells; under 8 the board is one object cut into no more pieces
    want = check(field(full), field(board), ONE, connectivity=4, max_objects=4096, max_pieces=4096, tag='board observed')
    assert want['pieces']['n_pieces'].tolist() == [[2178]] and want['pieces']['observed'][0, 0, 2177] == 2178
    want = check(field(board), field(full), ONE, connectivity=8, tag='board, 8')
    assert want['pieces']['n_pieces'].tolist() == [[1]] and want['pieces']['area'][0, 0, 0] == 2178


@pytest.mark.parametrize('connectivity, density', [(4, 0.65), (8, 0.5)])
def test_min_area_changes_the_overlap(connectivity, density):
    rng = np.random.default_rng(40 + connectivity)
    for shape in [(65, 67), (130, 5), (257, 259)]:
        maps = np.stack([field(rng.random(shape) < density, rng) for _ in range(2)])
        obs = field(rng.random(shape) < density, rng)
        wants = [check(maps, obs, ONE, connectivity=connectivity, min_area=a, max_objects=8192, max_pieces=16384, multi=shape[1] > 5,
                       tag=(shape, a)) for a in (1, 3)]
        cells = [int(w['pieces']['area'].sum(dtype=i8)) for w in wants]
        assert cells[1] < cells[0], (shape, 'no dropped object changed the overlap map', cells)


@pytest.mark.parametrize('n_y, n_x', [(2, 3), (65, 67), (5, 130), (1, 1023), (1023, 1)])
def test_value_classes_thresholds_and_domain(n_y, n_x):
    """Three blocks plus the observation at four thresholds in one call, out of the composite tests' pool: ties, NaN, both
    infinities, signed zeros, denormals; then a domain mask that cuts objects."""
    rng = np.random.default_rng(2000 * n_y + n_x)
    maps, obs = values(rng, (3, n_y, n_x)), values(rng, (n_y, n_x))
    maps[:, 0, 0] = obs[0, 0] = 3.0
    part = (rng.random((n_y, n_x)) < 0.7).astype(u1)
    part[0, 0] = 1
    for connectivity in (4, 8):
        for min_area in (1, 3) if n_y * n_x > 6 else (1,):
            kw = dict(connectivity=connectivity, min_area=min_area, max_objects=2048, max_pieces=2048)
            whole = check(maps, obs, FOUR, tag=('pool', connectivity, min_area), **kw)
            cut = check(maps, obs, FOUR, domain=part, tag=('pool, domain', connectivity, min_area), **kw)
            if n_y * n_x > 6 and min_area == 1:
                assert int(cut['pieces']['area'].sum(dtype=i8)) < int(whole['pieces']['area'].sum(dtype=i8))
            assert not whole['pieces']['n_pieces'][:, 3].any() or np.isinf(maps).any()       # (threshold +inf: only +inf cells)


def test_an_overlap_cut_by_the_domain():
    full = np.full((9, 70), 4.0, f4)
    dom = np.ones((9, 70), u1)
    dom[:, 64] = 0                                        # (the cut lies at a chunk border)
    want = check(full, full, ONE, domain=dom, connectivity=8, tag='cut')
    assert want['pieces']['n_pieces'].tolist() == [[2]] and want['pieces']['area'][0, 0, :2].tolist() == [9 * 64, 9 * 5]
    assert want['pieces']['bbox'][0, 0, :2].tolist() == [[0, 63, 0, 8], [65, 69, 0, 8]]
    # one forecast object over two observed ones and back: two pieces of two pairs; then one pair in two pieces
    obs = full.copy()
    obs[4, :] = nan
    want = check(full, obs, ONE, connectivity=4, tag='two observed objects')
    assert want['pieces']['n_pieces'].tolist() == [[2]] and want['pieces']['forecast'][0, 0, :2].tolist() == [1, 1]
    assert want['pieces']['observed'][0, 0, :2].tolist() == [1, 2] and want['covered'][0, 0, 0] == 8 * 70
    ring = full.copy()
    ring[4, 1:] = nan                                     # (the two halves hang together at x = 0)
    cutf = full.copy()
    cutf[:, 0] = nan
    want = check(cutf, ring, ONE, connectivity=4, multi=True, tag='one pair, two pieces')
    assert want['pieces']['n_pieces'].tolist() == [[2]] and want['pieces']['observed'][0, 0, :2].tolist() == [1, 1]


def test_overflow_of_max_pieces():
    board, full = pattern('checkerboard', (65, 67)), pattern('full', (65, 67))
    want = check(np.stack([field(board), field(full)]), field(full), ONE, connectivity=4, max_objects=4096, max_pieces=100, tag='pieces overflow')
    assert want['pieces']['n_pieces'].ravel().tolist() == [2178, 1] and want['pieces']['first'].shape == (2, 1, 100)
    assert want['pieces']['first'][0, 0].tolist() == [2 * k for k in range(34)] + [67 + 1 + 2 * k for k in range(33)] + [134 + 2 * k for k in range(33)]
    assert int(want['covered'][0, 0].sum()) == 2178 and want['covered_observed'][0, 0, 0] == 2178          # (complete whatever max_pieces is)
    small = field(pattern('checkerboard', (5, 7)))
    for rows in (17, 18, 19):
        assert check(small, field(pattern('full', (5, 7))), ONE, connectivity=4, max_pieces=rows, tag=rows)['pieces']['n_pieces'].tolist() == [[18]]


def test_overflow_of_max_objects():
    board, full = pattern('checkerboard', (65, 67)), pattern('full', (65, 67))
    want = check(np.stack([field(board), field(full)]), field(board), ONE, connectivity=4, max_objects=50, max_pieces=4096, tag='objects overflow')
    assert want['n_objects'].ravel().tolist() == [2178, 1] and want['observed']['n_objects'].tolist() == [2178]
    pc = want['pieces']
    assert pc['n_pieces'].ravel().tolist() == [2178, 2178] and pc['forecast'][0, 0, 2177] == 2178 and pc['observed'][1, 0, 2177] == 2178
    assert want['covered'].shape == (2, 1, 50) and (want['covered'][0] == 1).all() and want['covered'][1, 0].tolist() == [2178] + [0] * 49
    assert (want['covered_observed'] == 1).all()


def test_no_labels():
    rng = np.random.default_rng(21)
    maps = field(rng.random((2, 33, 70)) < 0.6, rng)
    obs = field(rng.random((33, 70)) < 0.6, rng)
    want = check(maps, obs, ONE, labels=False, multi=True, tag='no labels')
    assert 'labels' not in want and 'labels' not in want['observed']


def test_exact_sums_with_a_weight_table_beside_the_match():
    NB, OB = mods()
    rng = np.random.default_rng(22)
    maps = np.where(rng.random((2, 65, 67)) < 0.6, rng.random((2, 65, 67)) * 1e4 + 1.0, 0.1).astype(f4)
    obs = np.where(rng.random((65, 67)) < 0.6, rng.random((65, 67)) * 1e4 + 1.0, 0.1).astype(f4)
    maps[0, 3, 3] = inf                                   # (a skipped cell)
    for weight in (None, OB.zr_table()):
        kw = dict(sums=True, weight=weight, connectivity=8, min_area=2, max_objects=512, max_pieces=2048)
        want = check(maps, obs, [1.0, 100.0], multi=True, tag=('sums', weight is not None), **kw)
        assert (want['volume'] != 0).any() and (want['observed']['volume'] != 0).any() and int(want['field']['cells'].sum()) > 0
        assert (weight is not None) or int(want['skipped'].sum()) > 0


def test_stale_state_and_prefill():
    """Two different calls on one context, the second with fewer pieces and objects and smaller tables: nothing of the first may
    remain.  The hook prefills every output with 0xDEADBEEF, so the zero rows are the library's."""
    rng = np.random.default_rng(23)
    ctx = context()
    big = field(rng.random((3, 65, 67)) < 0.6, rng)
    first = check(big, big[0][::-1].copy(), ONE, connectivity=4, max_objects=2048, max_pieces=4096, multi=True, tag='first')
    assert int(first['pieces']['n_pieces'].min()) > 50
    small = np.full((1, 65, 67), -1.0, f4)
    small[0, 10:12, 10:20] = 3.0
    obs = np.full((65, 67), -1.0, f4)
    obs[11:30, 12:14] = 3.0
    second = check(small, obs, ONE, connectivity=4, max_objects=2048, max_pieces=4096, tag='second')
    assert second['pieces']['n_pieces'].tolist() == [[1]] and second['pieces']['area'][0, 0].tolist() == [2] + [0] * 4095
    assert second['pieces']['bbox'][0, 0, 0].tolist() == [12, 13, 11, 11] and second['covered'][0, 0].tolist() == [2] + [0] * 2047
    # max_pieces travels in the word that was pad_; a refused one is followed by a good call on the same context
    spec = spec_for(65, 67, ONE)
    seen = {}

    def tamper(f):
        o = f.objects.contents
        seen['pad'] = o.pad_
        o.pad_ = -1
    with pytest.raises(ValueError, match='cpol_objects: pad_'):
        ctx.fractions_maps(small, obs, spec.fractions, objects=spec, tamper=tamper)
    assert seen['pad'] == 1024
    check(small, obs, ONE, tag='after the refusal')


def test_refusals_leave_the_context_usable():
    from cosmo_pol_amd import _native as N
    NB, OB = mods()
    rng = np.random.default_rng(3)
    maps, obs = field(rng.random((2, 9, 70)) < 0.6, rng), field(rng.random((9, 70)) < 0.6, rng)
    spec = spec_for(9, 70, ONE)
    ctx = context()

    def set_to(name, value):
        def tamper(f):
            om = C.cast(f.objects, C.POINTER(N.ObjectsMatch)).contents
            if name == 'pad_':
                om.o.pad_ = value
            else:
                setattr(om, name, value)
        return tamper
    for name, value, what in (('pad_', -1, 'pad_ .* must lie in 0 ... 65535'), ('pad_', 65536, 'pad_ .* must lie in 0 ... 65535'),
                              ('n_pieces', None, 'n_pieces, pieces or covered is NULL'), ('pieces', None, 'n_pieces, pieces or covered is NULL'),
                              ('covered', None, 'n_pieces, pieces or covered is NULL')):
        with pytest.raises(ValueError, match='cpol_objects: ' + what):
            ctx.fractions_maps(maps, obs, spec.fractions, objects=spec, tamper=set_to(name, value))
        check(maps, obs, ONE, tag=('after the refusal', what))
    # a zero pad_ in the larger struct: off, the three arrays untouched, the cells as ever
    scores, got = ctx.fractions_maps(maps, obs, spec.fractions, objects=spec, tamper=set_to('pad_', 0))
    assert (got['pieces']['n_pieces'] == 0xDEADBEEF).all() and (got['covered'] == 0xDEADBEEF).all() and (got['pieces']['area'] == 0xDEADBEEF).all()
    same_cells(got, OB.cells(spec, maps, obs), 'pad_ 0')
    # the scratch above 1 GiB with the match where the call without it passes the check: 39 sources x 3 thresholds of 1023 x 1023
    # (refused before anything is uploaded: the maps are pages never touched)
    big = spec_for(1023, 1023, [1.0, 2.0, 3.0], max_objects=1, labels=False)
    assert OB.scratch_bytes(big, 38) > OB.MAX_SCRATCH_BYTES >= OB.scratch_bytes(spec_for(1023, 1023, [1.0, 2.0, 3.0], max_objects=1, match=False), 38)
    with pytest.raises(ValueError, match='cpol_objects: the labelling scratch, the sums\' accumulators and the piece scratch'):
        ctx.fractions_maps(np.zeros((38, 1023, 1023), f4), np.zeros((1023, 1023), f4), big.fractions, objects=big)
    check(maps, obs, ONE, tag='after the refused scratch')


@pytest.mark.parametrize('connectivity, density', [(4, 0.65), (8, 0.5)])
def test_the_largest_grid(connectivity, density):
    rng = np.random.default_rng(connectivity)
    b = rng.random((1023, 1023)) < density
    want = check(field(b, rng), field(b[::-1]), ONE, connectivity=connectivity, min_area=2, max_objects=65535, max_pieces=65535, labels=False,
                 tag='1023')
    assert int(want['pieces']['n_pieces'][0, 0]) > 10000
