"""The track of the object cells on the GPU, the kernels alone (k_track_bits, k_track_corr, k_track_shift, k_track_runs, the objects'
kernels on the track's piece arrays, k_track_attr and k_match_decode behind everything else through cpol_debug_read
"fractions_maps"): hand-built maps no sweep produces against objects.cells of the same maps.  Every number is a count, an integer
sum, an integer extreme or a comparison, so every comparison is np.array_equal: no tolerance anywhere, and no case is left out of
a comparison.  The hook prefills the track's outputs with 77, so the zero rows are the library's.  The cells, the exact sums, the
match and the scores of the same call are compared too, and with the call without the track: the track changes nothing of them."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

f4, u1, u4, u8, i4, i8 = np.float32, np.uint8, np.uint32, np.uint64, np.int32, np.int64
CELLS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')
PIECES = ('n_pieces', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'forecast', 'observed')
FLOATS = ('volume', 'moment_x', 'moment_y')
SCORES = ('diff2', 'forecast2', 'observed2', 'n_forecast', 'n_observed', 'n_domain')
TRACK = ('correlation', 'shift', 'n_pieces', 'pieces', 'covered')
ONE, FOUR = [0.75], [-np.inf, 0.75, 3.0, np.inf]
ROWS = 16                                                 # OBJ_TRACK_ROWS: the earlier rows a workgroup of k_track_corr takes
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
    kw.setdefault('track', True)
    if kw['track'] and 'shifts' not in kw:
        kw.setdefault('max_shift', 2)
    kw.setdefault('max_objects', 64)
    return OB.Objects(NB.Fractions(composite.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0)), 'ZH', thresholds, [0]), **kw)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: u4, 8: u8}[a.dtype.itemsize])


def same_rest(got, want, tag):
    """Everything but the track: the cells, the labels, the exact sums and the match of both sides."""
    for g, w in ((got, want), (got['observed'], want['observed'])):
        for k in CELLS + (('skipped',) if 'skipped' in w else ()):
            assert g[k].dtype == u4 and np.array_equal(g[k], w[k]), (tag, k)
        assert np.array_equal(bits(g['peak']), bits(w['peak'])), (tag, 'peak')
        assert ('labels' in g) == ('labels' in w) and ('volume' in g) == ('volume' in w), tag
        if 'labels' in w:
            assert np.array_equal(g['labels'], w['labels']), (tag, 'labels')
        if 'volume' in w:
            for k in FLOATS:
                assert np.array_equal(bits(g[k]), bits(w[k])) and np.array_equal(bits(g['field'][k]), bits(w['field'][k])), (tag, k)
            for k in ('cells', 'skipped'):
                assert np.array_equal(g['field'][k], w['field'][k]), (tag, 'field', k)
    assert ('pieces' in got) == ('pieces' in want), tag
    if 'pieces' in want:
        for k in PIECES:
            assert np.array_equal(got['pieces'][k], want['pieces'][k]), (tag, 'pieces', k)
        for k in ('covered', 'covered_observed'):
            assert np.array_equal(got[k], want[k]), (tag, k)


def same_track(got, want, tag):
    assert sorted(got['track']) == sorted(TRACK), tag
    for k in TRACK:
        g, w = got['track'][k], want['track'][k]
        if w is None:
            assert g is None and (got['track_correlation_buffer'] == 77).all(), (tag, 'a correlation that is not computed is not written')
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (tag, k, int((g != w).sum()), g.ravel()[:12], w.ravel()[:12])


def check(maps, thresholds, obs=None, domain=None, busy=True, tag='', **kw):
    """The device result of the hook against the rule; then the same call without the track: nothing else changed."""
    NB, OB = mods()
    obs = maps[-1] if obs is None else obs
    n_y, n_x = obs.shape
    spec = spec_for(n_y, n_x, thresholds, **kw)
    want = OB.cells(spec, maps, obs, domain)
    assert int(want['track']['n_pieces'].sum(dtype=i8)) > 0 or not busy, (tag, 'the rule itself finds no piece')
    ctx = context()
    scores, got = ctx.fractions_maps(maps, obs, spec.fractions, domain=domain, objects=spec)
    same_track(got, want, tag)
    same_rest(got, want, tag)
    tr = got['track']
    if int(tr['n_pieces'].max()) <= spec.max_track_pieces and int(got['n_objects'].max()) <= spec.max_objects:      # the invariants
        cells = tr['pieces'][..., OB.AREA].sum(axis=-1, dtype=u8)
        assert np.array_equal(cells, tr['covered'][..., 0, :].sum(axis=-1, dtype=u8)) and np.array_equal(cells, tr['covered'][..., 1, :].sum(axis=-1, dtype=u8)), tag
        assert (tr['covered'][..., 0, :] <= got['area'][:-1]).all() and (tr['covered'][..., 1, :] <= got['area'][1:]).all(), tag
    off = spec_for(n_y, n_x, thresholds, **dict(kw, track=False, max_shift=None, shifts=None, max_track_pieces=None))
    scores0, plain = ctx.fractions_maps(maps, obs, off.fractions, domain=domain, objects=off)
    assert 'track' not in plain and set(plain) | {'track', 'track_correlation_buffer'} == set(got) | {'track_correlation_buffer'}, tag
    same_rest(plain, got, (tag, 'track off'))
    for k in SCORES:
        assert np.array_equal(scores[k], scores0[k]) and np.array_equal(scores[k], NB.sums(spec.fractions, maps, obs, domain)[k]), (tag, k)
    return want


def field(binary, rng=None):
    """float32 values whose cells >= 0.75 are those of `binary`."""
    hi = np.full(binary.shape, 5.0, f4) if rng is None else (1.0 + rng.integers(0, 50, binary.shape)).astype(f4)
    return np.where(binary, hi, f4(-1.0)).astype(f4)


def moved(binary, dy, dx):
    _, OB = mods()
    return OB.shift_labels(binary.astype(i4), dy, dx) > 0


def frames(rng, n_blocks, n_y, n_x, step, density=0.35, noise=0.03):
    """Blocks that carry one random pattern along by `step` = (dy, dx) per block, with a little noise of their own."""
    base = rng.random((n_y, n_x)) < density
    base[n_y // 2, n_x // 2] = True
    return np.stack([moved(base, b * step[0], b * step[1]) | (rng.random((n_y, n_x)) < noise) for b in range(n_blocks)])


@pytest.mark.parametrize('n_x', [1, 2, 63, 64, 65, 129])
def test_shapes_and_reaches_equal_the_rule(n_x):
    """n_y: 1, 2 and one more than the rows a workgroup of k_track_corr takes; S: 0, 1, 2, 32 (beyond both sides of the small grids)."""
    rng = np.random.default_rng(n_x)
    pieces = 0
    for n_y in (1, 2, ROWS + 1):
        for S in (0, 1, 2, 32):
            step = (min(S, 1, n_y - 1), -min(S, 2, n_x - 1))
            binary = frames(rng, 3, n_y, n_x, step)
            for connectivity in (4, 8):
                want = check(field(binary, rng), ONE, busy=False, connectivity=connectivity, max_shift=S, max_track_pieces=64, tag=(n_y, n_x, S, connectivity))
                assert want['track']['correlation'].shape == (2, 1, 2 * S + 1, 2 * S + 1)
                pieces += int(want['track']['n_pieces'].sum())
                if S >= 2 and n_y > 2 and n_x > 2:
                    assert want['track']['shift'][:, 0].tolist() == [list(step)] * 2, (n_y, n_x, S, 'the rule does not find the step')
    assert pieces > 0


def test_one_cell_empty_and_full_maps():
    one = np.full((2, 1, 1), 2.0, f4)
    want = check(one, ONE, max_shift=32, tag='one cell')
    assert want['track']['n_pieces'].tolist() == [[1]] and want['track']['shift'].tolist() == [[[0, 0]]] and want['track']['correlation'].sum() == 1
    for shape in ((1, 130), (ROWS + 1, 65), (33, 129)):
        full, empty = np.full((3,) + shape, 2.0, f4), np.full((3,) + shape, -1.0, f4)
        for S in (0, 2, 32):
            want = check(full, ONE, max_shift=S, tag=('full', shape, S))
            d = np.arange(-S, S + 1)
            assert np.array_equal(want['track']['correlation'][0, 0], np.maximum(shape[0] - abs(d), 0)[:, None] * np.maximum(shape[1] - abs(d), 0)[None])
            assert want['track']['n_pieces'].tolist() == [[1], [1]] and not want['track']['shift'].any()
            want = check(empty, ONE, busy=False, max_shift=S, tag=('empty', shape, S))
            assert not want['track']['n_pieces'].any() and not want['track']['shift'].any() and not want['track']['correlation'].any()
        mixed = np.stack([full[0], empty[0], full[0]])
        assert not check(mixed, ONE, busy=False, max_shift=2, tag=('mixed', shape))['track']['n_pieces'].any()


def test_known_displacements_and_the_tie_order():
    rng = np.random.default_rng(7)
    base = np.zeros((100, 200), bool)
    base[40:52, 80:130] = rng.random((12, 50)) < 0.5
    for S, steps in ((8, [(0, 0), (3, -4), (-2, 5), (8, 8), (-8, -8), (8, -8)]), (32, [(32, -32), (-32, 32), (-17, 31)])):
        for dy, dx in steps:
            want = check(field(np.stack([base, moved(base, dy, dx)]), rng), ONE, max_shift=S, connectivity=8, max_objects=512, max_track_pieces=512,
                         tag=('moved', dy, dx))
            assert want['track']['shift'].tolist() == [[[dy, dx]]] and int(want['track']['covered'][0, 0, 0].sum()) == int(base.sum())
    # ties: one cell against two cells at equal distance: the smallest dy wins, then the smallest dx
    e = np.zeros((9, 70), bool)
    e[4, 64] = True
    for cells, shift in (([(3, 62), (5, 66)], (-1, -2)), ([(2, 65), (5, 62)], (-2, 1)), ([(4, 66), (4, 62)], (0, -2)), ([(6, 64), (4, 62)], (0, -2)),
                         ([(6, 64), (2, 64)], (-2, 0))):
        l = np.zeros((9, 70), bool)
        for y, x in cells:
            l[y, x] = True
        want = check(field(np.stack([e, l])), ONE, max_shift=3, tag=('tie', cells))
        assert want['track']['shift'].tolist() == [[list(shift)]] and want['track']['n_pieces'].tolist() == [[1]]


def test_objects_that_cross_a_chunk_boundary_only_after_the_shift():
    e = np.zeros((5, 200), bool)
    e[1:3, 50:62] = True                                  # inside the first 64-cell chunk
    e[3, 120:127] = True
    for dx in (4, 10, 70, -50):
        l = moved(e, 1, dx)
        assert l.any()
        for kw in ({'max_shift': 0}, {'shifts': [1, dx]}, {'shifts': [0, dx]}):
            want = check(field(np.stack([e, l])), ONE, busy='shifts' in kw, connectivity=4, tag=('cross', dx, sorted(kw)), **kw)
            if kw.get('shifts') == [1, dx]:
                assert want['track']['n_pieces'].tolist() == [[2]] and int(want['track']['covered'][0, 0, 1].sum()) == int(l.sum())
    want = check(field(np.stack([e, moved(e, 1, 10)])), ONE, max_shift=12, tag='cross, found')
    assert want['track']['shift'].tolist() == [[[1, 10]]] and want['track']['pieces'][0, 0, 0, 4:8].tolist() == [60, 71, 2, 3]


def test_given_shifts():
    rng = np.random.default_rng(8)
    binary = frames(rng, 4, 33, 130, (2, -3), density=0.3)
    maps = field(binary, rng)
    for shifts in ([2, -3], [-2, 3], [0, 0], [1023, -1023], [-1023, 1023], [32, 129], [-33, 0], [0, 130],
                   np.array([[[2, -3], [1, 1]], [[-5, 70], [0, -64]], [[40, 0], [1023, 1023]]])):
        want = check(maps, [0.75, 20.0], busy=False, shifts=shifts, connectivity=8, max_track_pieces=2048, max_objects=2048, tag=('given', np.shape(shifts)))
        assert want['track']['correlation'] is None and np.array_equal(want['track']['shift'], np.broadcast_to(np.asarray(shifts, i4), (3, 2, 2)))
        if np.abs(np.asarray(shifts)).max() > 130:
            assert not want['track']['n_pieces'].any() or np.ndim(shifts) == 3    # (a shift that moves every object wholly outside)
    assert check(maps, [0.75, 20.0], shifts=[2, -3], connectivity=8, max_track_pieces=2048, max_objects=2048)['track']['n_pieces'].min() > 10


@pytest.mark.parametrize('n_blocks, thresholds', [(2, ONE), (3, FOUR), (9, ONE), (9, FOUR)])
def test_blocks_thresholds_min_area_and_overflows(n_blocks, thresholds):
    rng = np.random.default_rng(10 * n_blocks + len(thresholds))
    binary = frames(rng, n_blocks, ROWS + 3, 131, (1, 2), density=0.45, noise=0.05)
    maps = field(binary, rng)
    maps[:, 0, 0] = np.inf                                # (threshold +inf: only these cells)
    dom = (rng.random(binary.shape[1:]) < 0.9).astype(u1)
    dom[0, 0] = 1
    base = check(maps, thresholds, connectivity=4, max_shift=3, max_objects=2048, max_track_pieces=4096, tag='whole')
    assert base['track']['n_pieces'].shape == (n_blocks - 1, len(thresholds)) and int(base['track']['n_pieces'].min()) > 0
    check(maps, thresholds, domain=dom, connectivity=8, max_shift=3, max_objects=2048, max_track_pieces=4096, tag='domain')
    # min_area drops objects: they must not appear in Ke, so the correlation and the overlap shrink
    kept = check(maps, thresholds, connectivity=4, min_area=4, max_shift=3, max_objects=2048, max_track_pieces=4096, tag='min_area')
    assert int(kept['track']['correlation'].sum(dtype=i8)) < int(base['track']['correlation'].sum(dtype=i8))
    assert int(kept['track']['covered'].sum(dtype=i8)) < int(base['track']['covered'].sum(dtype=i8))
    # more objects than max_objects, more pieces than max_track_pieces (and a single row): the true counts, covered complete
    few = check(maps, thresholds, connectivity=4, max_shift=3, max_objects=5, max_track_pieces=3, tag='overflow')
    assert int(few['n_objects'].max()) > 5 and int(few['track']['n_pieces'].max()) > 3
    assert np.array_equal(few['track']['n_pieces'], base['track']['n_pieces']) and np.array_equal(few['track']['pieces'], base['track']['pieces'][:, :, :3])
    assert np.array_equal(few['track']['covered'], base['track']['covered'][..., :5]) and np.array_equal(few['track']['shift'], base['track']['shift'])
    one = check(maps, thresholds, connectivity=8, max_shift=3, max_objects=2048, max_track_pieces=1, tag='one row')
    assert one['track']['pieces'].shape[2] == 1 and int(one['track']['n_pieces'].max()) > 1


def test_labels_sums_and_match_beside_the_track():
    _, OB = mods()
    rng = np.random.default_rng(12)
    binary = frames(rng, 3, 33, 67, (1, -1), density=0.4)
    maps = np.where(binary, rng.random(binary.shape) * 1e4 + 1.0, 0.1).astype(f4)
    obs = np.where(moved(binary[0], 2, 2), 7.0, 0.1).astype(f4)
    for kw in ({'labels': False}, {'sums': True}, {'sums': True, 'weight': OB.zr_table()}, {'match': True, 'max_pieces': 512},
               {'labels': False, 'sums': True, 'match': True, 'max_pieces': 3}):
        want = check(maps, [1.0, 100.0], obs=obs, connectivity=8, min_area=2, max_shift=2, max_objects=512, max_track_pieces=512,
                     tag=sorted(kw), **kw)
        assert ('pieces' in want) == ('match' in kw) and ('volume' in want) == ('sums' in kw) and ('labels' in want) == ('labels' not in kw)
        assert int(want['track']['n_pieces'].min()) > 0


def test_prefill_stale_state_and_a_correlation_that_is_not_wanted():
    from cosmo_pol_amd import _native as N
    _, OB = mods()
    rng = np.random.default_rng(13)
    ctx = context()
    big = field(frames(rng, 5, 65, 131, (1, 1), density=0.5), rng)
    first = check(big, ONE, connectivity=4, max_shift=4, max_objects=2048, max_track_pieces=4096, tag='first')
    assert int(first['track']['n_pieces'].min()) > 50
    small = np.full((2, 65, 131), -1.0, f4)
    small[0, 10:12, 10:20] = small[1, 11:13, 13:23] = 3.0
    second = check(small, ONE, connectivity=4, max_shift=4, max_objects=2048, max_track_pieces=4096, tag='second')
    assert second['track']['n_pieces'].tolist() == [[1]] and second['track']['shift'].tolist() == [[[1, 3]]]
    assert second['track']['pieces'][0, 0, :, OB.AREA].tolist() == [20] + [0] * 4095 and second['track']['covered'][0, 0].tolist() == [[20] + [0] * 2047] * 2
    # a NULL correlation with max_shift >= 0: the counters lie in the scratch, the caller's array is not written, the rest as ever
    spec = spec_for(65, 131, ONE, connectivity=4, max_shift=4, max_objects=2048, max_track_pieces=4096)

    def unwanted(f):
        C.cast(f.objects, C.POINTER(N.ObjectsTrack)).contents.correlation = None
    _, got = ctx.fractions_maps(big, big[-1], spec.fractions, objects=spec, tamper=unwanted)
    assert (got['track']['correlation'] == 77).all()
    for k in TRACK[1:]:
        assert np.array_equal(got['track'][k], first['track'][k]), k


def test_refusals_leave_the_context_usable():
    from cosmo_pol_amd import _native as N
    _, OB = mods()
    rng = np.random.default_rng(3)
    maps = field(frames(rng, 3, 9, 70, (0, 1)), rng)
    spec, given = spec_for(9, 70, ONE), spec_for(9, 70, ONE, shifts=[1, 1])
    ctx = context()

    def set_to(name, value):
        def tamper(f):
            ot = C.cast(f.objects, C.POINTER(N.ObjectsTrack)).contents
            if name == 'pad_':
                ot.m.o.pad_ = value
            elif name == 'shifts':
                a = np.full((2, 1, 2), value, i4)
                ot.shifts_in = a.ctypes.data
                return a
            else:
                setattr(ot, name, value)
        return tamper
    null = 'shift, n_pieces, pieces or covered of the track is NULL'
    for sp, name, value, what in ((spec, 'max_shift', 33, 'max_shift must lie in -1 ... 32'), (spec, 'max_shift', -2, 'max_shift must lie in -1 ... 32'),
                                  (spec, 'max_shift', -1, 'max_shift == -1 needs shifts_in'), (given, 'max_shift', 2, 'shifts_in belongs to max_shift == -1'),
                                  (given, 'shifts', 1024, 'a given shift must lie in -1023 ... 1023'),
                                  (given, 'shifts', -1024, 'a given shift must lie in -1023 ... 1023'),
                                  (spec, 'max_pieces', 0, 'max_pieces of the track must lie in 1 ... 65535'),
                                  (spec, 'max_pieces', 65536, 'max_pieces of the track must lie in 1 ... 65535'),
                                  (spec, 'shift', None, null), (spec, 'n_pieces', None, null), (spec, 'pieces', None, null), (spec, 'covered', None, null),
                                  (spec, 'pad_', -1, 'pad_ .* must lie in 0 ... 65535'), (spec, 'pad_', N.OBJ_TRACK | 65536, 'pad_ .* must lie in 0 ... 65535'),
                                  (spec, 'pad_', 1 << 29, 'pad_ .* must lie in 0 ... 65535')):
        with pytest.raises(ValueError, match='cpol_objects: ' + what):
            ctx.fractions_maps(maps, maps[0], sp.fractions, objects=sp, tamper=set_to(name, value))
        check(maps, ONE, tag=('after the refusal', what))
    # one block
    with pytest.raises(ValueError, match='cpol_objects: the track needs at least two blocks'):
        ctx.fractions_maps(maps[:1], maps[0], spec.fractions, objects=spec)
    with pytest.raises(ValueError, match='cpol_objects: the track needs at least two blocks'):
        ctx.fractions_maps(maps[:1], maps[0], given.fractions, objects=given)
    check(maps, ONE, shifts=[1023, -1023], busy=False, tag='after one block')
    # a pad_ without the bit in the larger struct: the track is off, its arrays untouched, the cells as ever
    _, got = ctx.fractions_maps(maps, maps[0], spec.fractions, objects=spec, tamper=set_to('pad_', 0))
    assert all((got['track'][k] == 77).all() for k in TRACK)
    same_rest(got, OB.cells(spec_for(9, 70, ONE, track=False), maps, maps[0]), 'pad_ 0')
    # the scratch above 1 GiB with the track where the call without it passes the check: 31 sources x 3 thresholds of 1023 x 1023
    # (refused before anything is uploaded: the maps are pages never touched)
    big = spec_for(1023, 1023, [1.0, 2.0, 3.0], max_objects=1, labels=False)
    assert OB.scratch_bytes(big, 30) > OB.MAX_SCRATCH_BYTES >= OB.scratch_bytes(spec_for(1023, 1023, [1.0, 2.0, 3.0], max_objects=1, track=False), 30)
    with pytest.raises(ValueError, match='cpol_objects: the scratch with the track\'s masks and piece maps must be at most 1 GiB'):
        ctx.fractions_maps(np.zeros((30, 1023, 1023), f4), np.zeros((1023, 1023), f4), big.fractions, objects=big)
    check(maps, ONE, tag='after the refused scratch')


@pytest.mark.parametrize('connectivity, density', [(4, 0.62), (8, 0.45)])
def test_the_largest_grid(connectivity, density):
    rng = np.random.default_rng(connectivity)
    b = rng.random((1023, 1023)) < density
    want = check(field(np.stack([b, moved(b, -3, 2)]), rng), ONE, connectivity=connectivity, min_area=2, max_shift=4, max_objects=65535,
                 max_track_pieces=65535, labels=False, tag='1023')
    assert want['track']['shift'].tolist() == [[[-3, 2]]] and int(want['track']['n_pieces'][0, 0]) > 1000
