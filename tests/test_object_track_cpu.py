"""The track of the object cells without a GPU: the rule (cosmo_pol_amd/objects.py: `correlation_of_pair`, `shift_of`,
`shift_labels`, `track_of_maps`, `cells` with track) against a literal triple loop, known displacements, the tie order and closed
forms; `track_of_maps` against `pieces_of_map` on hand-shifted label maps; the host folds `links`, `tracks` and `motion` on a
hand-made scene whose ids are written out; every ValueError of the spec, its key, repr and scratch size; the product object
`Cells`; the ctypes mirror of cpol_objects_track against the header; and the host header (cosmo_pol_amd/csrc/cpol_obj.h) through
tests/c_host/obj_track_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program of its own.  All
comparisons are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import neighbourhood as NB
from cosmo_pol_amd import objects as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f4, u1, u4, i4, i8 = np.float32, np.uint8, np.uint32, np.int32, np.int64
TRACK_KEYS = ['correlation', 'covered', 'n_pieces', 'pieces', 'shift']


def comp(n_x, n_y):
    return CP.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0))


def spec_of(n_x, n_y, thresholds=(0.5,), **kw):
    kw.setdefault('track', True)
    if kw['track'] and 'shifts' not in kw:
        kw.setdefault('max_shift', 2)
    return OB.Objects(NB.Fractions(comp(n_x, n_y), 'ZH', list(thresholds), [0]), **kw)


def literal_correlation(ke, kl, S):
    n_y, n_x = ke.shape
    C_ = np.zeros((2 * S + 1, 2 * S + 1), u4)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            for y in range(n_y):
                for x in range(n_x):
                    if ke[y, x] and 0 <= y + dy < n_y and 0 <= x + dx < n_x and kl[y + dy, x + dx]:
                        C_[dy + S, dx + S] += 1
    return C_


def blobs(shape, rng, n=4):
    out = np.zeros(shape, bool)
    for _ in range(n):
        y, x = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        out[y:y + rng.integers(1, 4), x:x + rng.integers(1, 6)] = True
    return out


def moved(binary, dy, dx):
    return OB.shift_labels(binary.astype(i4), dy, dx) > 0


# ---------------------------------------------------------------------------------------------------- the rule
def test_correlation_against_the_triple_loop():
    rng = np.random.default_rng(1)
    for shape in [(1, 1), (1, 7), (6, 1), (2, 3), (5, 9), (7, 70)]:
        for S in (0, 1, 2, 9):
            ke, kl = rng.random(shape) < 0.5, rng.random(shape) < 0.5
            got = OB.correlation_of_pair(ke.astype(i4) * 3, kl.astype(i4) * 5, S)
            assert got.dtype == u4 and got.shape == (2 * S + 1, 2 * S + 1) and np.array_equal(got, literal_correlation(ke, kl, S)), (shape, S)
    with pytest.raises(ValueError, match='two maps of one shape'):
        OB.correlation_of_pair(np.zeros((2, 2), i4), np.zeros((2, 3), i4), 1)


def test_full_and_empty_maps_closed_forms():
    for n_y, n_x, S in ((5, 7, 2), (3, 2, 4), (1, 1, 1), (9, 70, 32)):
        full = np.ones((n_y, n_x), i4)
        got = OB.correlation_of_pair(full, full, S)
        d = np.arange(-S, S + 1)
        want = np.maximum(n_y - np.abs(d), 0)[:, None] * np.maximum(n_x - np.abs(d), 0)[None]
        assert np.array_equal(got, want) and OB.shift_of(got) == (0, 0)
        empty = OB.correlation_of_pair(full * 0, full, S)
        assert not empty.any() and OB.shift_of(empty) == (0, 0)


def test_known_shifts_come_back():
    rng = np.random.default_rng(2)
    S = 5
    base = np.zeros((40, 90), bool)
    base[15:25, 30:60] = blobs((10, 30), rng, 8)
    assert base.any()
    for dy, dx in [(0, 0), (1, 0), (0, -1), (3, -4), (-2, 5), (S, S), (-S, -S), (S, -S), (-S, S)]:
        table = OB.correlation_of_pair(base, moved(base, dy, dx), S)
        assert OB.shift_of(table) == (dy, dx) and table[dy + S, dx + S] == base.sum(), (dy, dx)


def test_the_tie_order():
    S = 2
    table = np.zeros((5, 5), u4)
    assert OB.shift_of(table) == (0, 0)
    table[S + 1, S + 2] = table[S - 1, S - 2] = table[S + 2, S + 1] = table[S - 2, S - 1] = 7      # four offsets at distance 5
    assert OB.shift_of(table) == (-2, -1)                 # the smallest dy, whatever dx
    table[S - 2, S - 1] = 0
    assert OB.shift_of(table) == (-1, -2)
    table[S - 1, S - 2] = 0
    assert OB.shift_of(table) == (1, 2)
    table[S, S + 1] = table[S, S - 1] = 7                 # distance 1 beats distance 5; dy equal: the smallest dx
    assert OB.shift_of(table) == (0, -1)
    table[S - 1, S] = 7
    assert OB.shift_of(table) == (-1, 0)
    table[S + 2, S + 2] = 8                               # the largest count beats every distance
    assert OB.shift_of(table) == (2, 2)
    with pytest.raises(ValueError, match='shift_of'):
        OB.shift_of(np.zeros((4, 4), u4))


def test_shift_labels():
    le = np.arange(1, 13, dtype=i4).reshape(3, 4)
    assert np.array_equal(OB.shift_labels(le, 0, 0), le)
    assert OB.shift_labels(le, 1, -2).tolist() == [[0, 0, 0, 0], [3, 4, 0, 0], [7, 8, 0, 0]]
    assert OB.shift_labels(le, -2, 1).tolist() == [[0, 9, 10, 11], [0, 0, 0, 0], [0, 0, 0, 0]]
    for dy, dx in ((3, 0), (0, 4), (-3, 0), (0, -4), (1023, -1023)):
        assert not OB.shift_labels(le, dy, dx).any()


def test_track_of_maps_equals_pieces_of_map_on_hand_shifted_maps():
    rng = np.random.default_rng(3)
    n_y, n_x, B = 17, 70, 4
    frames = [blobs((n_y, n_x), rng, 12) for _ in range(B)]
    maps = np.stack([np.where(b, 2.0, -1.0) for b in frames]).astype(f4)
    maps[1][frames[1]] = 0.7                              # (between the two thresholds)
    for connectivity, min_area in ((4, 1), (8, 1), (8, 3)):
        for kw in ({'max_shift': 3}, {'max_shift': 0}, {'shifts': [1, -2]}, {'shifts': np.array([[[0, 0], [5, 5]], [[-1, 0], [0, 1]], [[2, 2], [-70, 0]]])}):
            spec = spec_of(n_x, n_y, (0.5, 1.0), connectivity=connectivity, min_area=min_area, max_objects=6, max_track_pieces=5, **kw)
            tr = OB.track_of_maps(spec, maps)
            assert sorted(tr) == TRACK_KEYS and tr['shift'].shape == (B - 1, 2, 2) and tr['shift'].dtype == i4
            assert tr['pieces'].shape == (B - 1, 2, 5, OB.WORDS) and tr['covered'].shape == (B - 1, 2, 2, 6) and tr['n_pieces'].dtype == u4
            assert (tr['correlation'] is None) == ('shifts' in kw)
            res = OB.cells(spec, maps, maps[0])
            for k in TRACK_KEYS:
                assert (tr[k] is None and res['track'][k] is None) or np.array_equal(tr[k], res['track'][k]), k
            big = OB.cells(spec_of(n_x, n_y, (0.5, 1.0), connectivity=connectivity, min_area=min_area, max_objects=512, max_track_pieces=512, **kw),
                           maps, maps[0])
            for p in range(B - 1):
                for t in range(2):
                    le, ll = res['labels'][p, t], res['labels'][p + 1, t]
                    if 'max_shift' in kw:
                        assert np.array_equal(tr['correlation'][p, t], literal_correlation(le > 0, ll > 0, kw['max_shift']))
                        assert tuple(tr['shift'][p, t]) == OB.shift_of(tr['correlation'][p, t])
                    else:
                        assert tuple(tr['shift'][p, t]) == tuple(np.broadcast_to(kw['shifts'], (B - 1, 2, 2))[p, t])
                    dy, dx = tr['shift'][p, t]
                    hand = np.zeros_like(le)
                    for y in range(n_y):
                        for x in range(n_x):
                            if 0 <= y - dy < n_y and 0 <= x - dx < n_x:
                                hand[y, x] = le[y - dy, x - dx]
                    n, pieces, covered = OB.pieces_of_map(hand, ll, connectivity, 5, 6)
                    assert tr['n_pieces'][p, t] == n and np.array_equal(tr['pieces'][p, t], pieces) and np.array_equal(tr['covered'][p, t], covered)
                    # the invariants, where nothing overflows
                    bt = big['track']
                    cells = int(((hand > 0) & (ll > 0)).sum())
                    assert bt['pieces'][p, t, :, OB.AREA].sum() == bt['covered'][p, t, 0].sum() == bt['covered'][p, t, 1].sum() == cells
                    assert (bt['covered'][p, t, 0] <= big['area'][p, t]).all() and (bt['covered'][p, t, 1] <= big['area'][p + 1, t]).all()
    with pytest.raises(ValueError, match='at least two'):
        OB.track_of_maps(spec_of(n_x, n_y), maps[:1])
    with pytest.raises(ValueError, match='does not broadcast'):
        OB.track_of_maps(spec_of(n_x, n_y, shifts=np.zeros((2, 1, 2), i4)), maps)
    with pytest.raises(ValueError, match='has no track'):
        OB.track_of_maps(spec_of(n_x, n_y, track=False), maps)
    off = OB.cells(spec_of(n_x, n_y, track=False), maps, maps[0])
    assert 'track' not in off and set(off) | {'track'} == set(OB.cells(spec_of(n_x, n_y), maps, maps[0]))


# ---------------------------------------------------------------------------------------------------- the host folds
def scene():
    """Four blocks of 8 x 24 cells, no motion (max_shift 0).
    block 0: A (cols 0-5), B (cols 8-11), C (cols 14-15)            tracks 1, 2, 3
    block 1: A stays; B splits into B1 (cols 8-9, rows 0-3: 8 cells) and B2 (cols 11, rows 0-3: 4 cells); C is gone (a death);
             D is born at cols 20-22                                  A: 1, B1: 2 (the larger overlap inherits), B2: 4 (parent 2), D: 5
    block 2: A and B1 merge into one object M (cols 0-9); B2 stays; D stays
             M's predecessor is A (24 cells against 8): M: 1; B1's track 2 ends, merged into 1; B2: 4, D: 5
    block 3: everything but D is gone."""
    z = np.zeros((4, 8, 24), f4)
    z[0, 0:4, 0:6] = z[0, 0:4, 8:12] = z[0, 0:4, 14:16] = 1
    z[1, 0:4, 0:6] = z[1, 0:4, 8:10] = z[1, 0:4, 11] = z[1, 0:4, 20:23] = 1
    z[2, 0:4, 0:10] = z[2, 0:4, 11] = z[2, 0:4, 20:23] = 1
    z[3, 0:4, 20:23] = 1
    return z


def test_tracks_links_and_motion_on_a_hand_made_scene():
    z = scene()
    res = OB.cells(spec_of(24, 8, max_shift=0, max_objects=8), z, z[0])
    assert res['n_objects'][:, 0].tolist() == [3, 4, 3, 1] and not res['track']['shift'].any()
    L = OB.links(res, 0)
    assert (L['earlier'].tolist(), L['later'].tolist(), L['area'].tolist()) == ([1, 2, 2], [1, 2, 3], [24, 8, 4]) and all(v.dtype == i8 for v in L.values())
    L = OB.links(res, 1)
    assert (L['earlier'].tolist(), L['later'].tolist(), L['area'].tolist(), L['pieces'].tolist()) == ([1, 2, 3, 4], [1, 1, 2, 3], [24, 8, 4, 12], [1, 1, 1, 1])
    tk = OB.tracks(res)
    assert [a.tolist() for a in tk['track_id']] == [[1, 2, 3], [1, 2, 4, 5], [1, 4, 5], [5]]
    assert tk['birth'].tolist() == [0, 0, 0, 1, 1] and tk['death'].tolist() == [2, 1, 0, 2, 3]
    assert tk['parent'].tolist() == [0, 0, 0, 2, 0] and tk['merged_into'].tolist() == [0, 1, 0, 0, 0]
    assert [a.tolist() for a in tk['inherited']] == [[[1, 1], [2, 2]], [[1, 1], [3, 2], [4, 3]], [[3, 1]]]
    # min_cover: the split-off B2 covers 4 of its 4 cells but B1's overlap with M is 8 of min(8, 40): both stay at 1.0; the link of B
    # (16 cells) to B2 (4 cells) has 4 >= 1.0 * 4
    assert OB.links(res, 0, min_cover=1.0)['area'].tolist() == [24, 8, 4]
    # a partial overlap drops out under min_cover: A moved so that it keeps 2 of its 6 columns
    y = np.zeros((2, 8, 24), f4)
    y[0, 0:4, 0:6] = y[1, 0:4, 4:10] = 1
    part = OB.cells(spec_of(24, 8, max_shift=0, max_objects=8), y, y[0])
    assert OB.links(part, 0)['area'].tolist() == [8] and OB.links(part, 0, min_cover=0.5)['area'].size == 0
    assert OB.links(part, 0, min_cover=1 / 3)['area'].tolist() == [8]
    tp = OB.tracks(part, min_cover=0.5)
    assert [a.tolist() for a in tp['track_id']] == [[1], [2]] and tp['parent'].tolist() == [0, 0] and tp['merged_into'].tolist() == [0, 0]
    assert [a.tolist() for a in OB.tracks(part)['track_id']] == [[1], [1]]
    # ties: two later objects of equal overlap with one earlier object: the smaller number inherits, the other one is a split
    w = np.zeros((2, 3, 9), f4)
    w[0, 0, 0:9] = 1
    w[1, 0, 0:3] = w[1, 0, 5:8] = 1
    tie = OB.tracks(OB.cells(spec_of(9, 3, max_shift=0), w, w[0]))
    assert [a.tolist() for a in tie['track_id']] == [[1], [1, 2]] and tie['parent'].tolist() == [0, 1]
    # motion: the found shift, and the centroids' displacement per inherited link
    base = np.zeros((16, 30), f4)
    base[2:5, 3:9] = base[8:10, 20:24] = 1
    mv = np.stack([base, OB.shift_labels(base, 1, 2), OB.shift_labels(base, 3, 1)])
    m = OB.motion(OB.cells(spec_of(30, 16, max_shift=4), mv, mv[0]))
    assert m['shift'].tolist() == [[1, 2], [2, -1]] and m['shift'].dtype == i4
    assert m['links'][0]['earlier'].tolist() == [1, 2] and m['links'][0]['displacement'].tolist() == [[1.0, 2.0], [1.0, 2.0]]
    assert m['links'][1]['displacement'].tolist() == [[2.0, -1.0], [2.0, -1.0]]
    # incomplete pieces: the links would be partial
    few = OB.cells(spec_of(24, 8, max_shift=0, max_objects=8, max_track_pieces=2), z, z[0])
    assert few['track']['n_pieces'][:, 0].tolist() == [3, 4, 1] and few['track']['pieces'].shape == (3, 1, 2, OB.WORDS)
    for fold in (lambda r: OB.links(r, 0), OB.tracks, OB.motion):
        with pytest.raises(ValueError, match='a partial fold is not returned'):
            fold(few)
    assert OB.links(few, 2)['area'].tolist() == [12]
    plain = OB.cells(spec_of(24, 8, track=False), z, z[0])
    for fold in (lambda r: OB.links(r, 0), OB.tracks, OB.motion):
        with pytest.raises(ValueError, match='has no track'):
            fold(plain)
    with pytest.raises(ValueError, match='threshold index outside'):
        OB.tracks(res, 1)
    with pytest.raises(ValueError, match='pair outside'):
        OB.links(res, 3)


# ---------------------------------------------------------------------------------------------------- the spec
def test_spec_refusals_identity_key_and_scratch():
    fr = NB.Fractions(comp(70, 3), 'ZH', [0.1, 0.2], [1, 2])
    off, on = OB.Objects(fr), OB.Objects(fr, track=True, max_shift=8)
    assert off.key == (fr.key, 4, 1, 1024, True) and (off.track, off.max_shift, off.shifts, off.max_track_pieces) == (False, None, None, None)
    assert 'track' not in repr(off)
    assert (on.track, on.max_shift, on.shifts, on.max_track_pieces) == (True, 8, None, 1024)
    assert on.key == off.key + ('track', 8, None, 1024) and repr(on).endswith(', track=True, max_shift=8, max_track_pieces=1024)')
    assert on != off and on == OB.Objects(fr, track=True, max_shift=8, max_track_pieces=1024) and hash(on) == hash(OB.Objects(fr, track=True, max_shift=8))
    assert on != OB.Objects(fr, track=True, max_shift=7) and OB.Objects(fr, max_objects=9, track=True, max_shift=0).max_track_pieces == 9
    given = OB.Objects(fr, track=True, shifts=[[3, -4]], max_track_pieces=5, match=True, sums=True)
    assert given.shifts.dtype == i4 and given.shifts.shape == (1, 2) and given.max_shift is None
    assert given.key == (fr.key, 4, 1, 1024, True, True, None, 'match', 1024, 'track', None, ((1, 2), np.array([3, -4], i4).tobytes()), 5)
    assert 'match=True, max_pieces=1024, track=True, shifts=<1x2>, max_track_pieces=5' in repr(given)
    assert given != OB.Objects(fr, track=True, shifts=[[3, -3]], max_track_pieces=5, match=True, sums=True)
    for kw, text in (({'max_shift': 2}, 'max_shift: belongs to track=True'), ({'shifts': [0, 0]}, 'shifts: belongs to track=True'),
                     ({'max_track_pieces': 5}, 'max_track_pieces: belongs to track=True'),
                     ({'track': True}, 'exactly one of max_shift and shifts'), ({'track': True, 'max_shift': 1, 'shifts': [0, 0]}, 'exactly one of'),
                     ({'track': True, 'max_shift': -1}, 'max_shift must lie in 0 ... 32'), ({'track': True, 'max_shift': 33}, 'max_shift must lie in'),
                     ({'track': True, 'max_shift': 1.0}, 'max_shift: an integer'), ({'track': True, 'max_shift': True}, 'max_shift: an integer'),
                     ({'track': True, 'shifts': [1024, 0]}, 'at most 1023'), ({'track': True, 'shifts': [0, -1024]}, 'at most 1023'),
                     ({'track': True, 'shifts': [0.5, 0]}, 'shifts: integers'), ({'track': True, 'shifts': [1, 2, 3]}, 'shifts: integers'),
                     ({'track': True, 'shifts': np.zeros((1, 1, 1, 2), i4)}, 'shifts: integers'), ({'track': True, 'shifts': 3}, 'shifts: integers'),
                     ({'track': True, 'max_shift': 1, 'max_track_pieces': 0}, 'max_track_pieces must lie in'),
                     ({'track': True, 'max_shift': 1, 'max_track_pieces': 65536}, 'max_track_pieces must lie in'),
                     ({'track': True, 'max_shift': 1, 'max_track_pieces': 2.0}, 'max_track_pieces: an integer')):
        with pytest.raises(ValueError, match=text):
            OB.Objects(fr, **kw)
    assert OB.Objects(fr, track=True, shifts=[1023, -1023]).shifts.tolist() == [1023, -1023]
    # the shape of given shifts is checked at the call, where P is known
    assert OB.shifts_of_call(given, 3).tolist() == [[[3, -4]] * 2] * 2
    with pytest.raises(ValueError, match='does not broadcast'):
        OB.shifts_of_call(OB.Objects(fr, track=True, shifts=np.zeros((3, 2, 2), i4)), 3)
    with pytest.raises(ValueError, match='at least two'):
        OB.shifts_of_call(given, 1)
    # the scratch: the packed masks of the blocks and the piece maps of the pairs behind everything else, 8-byte aligned
    per = (2 * 210 + 3) * 4
    assert OB.scratch_bytes(off, 3) == 4 * 2 * per
    assert OB.scratch_bytes(on, 3) == 4 * 2 * per + 3 * 2 * 3 * 2 * 8 + 2 * 2 * per
    both = OB.Objects(fr, match=True, track=True, max_shift=1)
    assert OB.scratch_bytes(both, 3) == OB.scratch_bytes(OB.Objects(fr, match=True), 3) + 3 * 2 * 3 * 2 * 8 + 2 * 2 * per
    odd = OB.Objects(NB.Fractions(comp(3, 3), 'ZH', [0.1], [0]), track=True, max_shift=1)
    assert OB.scratch_bytes(odd, 2) == (3 * 21 * 4 + 7) // 8 * 8 + 2 * 3 * 8 + 21 * 4


# ---------------------------------------------------------------------------------------------------- the product object
def attach(product, az, n_gates, n_members=None, take=None):
    structs, keep = product.attach(N, az, n_gates, n_members, True, True, ['U', 'V', 'W', 'T'], take)
    return structs


def test_cells_arrays_binding_finish_and_refusals():
    c = CP.Composite(['KDP', 'ZH'], [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0], products=('max', 'lowest'))      # a 2 x 3 grid
    fr = NB.Fractions(c, 'KDP', [0.5, 1.5], [0, 1, 4], plane='lowest')
    obs = np.arange(6, dtype=f4).reshape(2, 3)

    def take(block):
        return [np.zeros(sh, dt) for _, dt, sh in block], [0x77000 + 64 * i for i in range(len(block))]
    az4 = np.arange(4.0)
    spec = OB.Objects(fr, connectivity=8, max_objects=5, match=True, max_pieces=7, track=True, max_shift=2, max_track_pieces=3)
    p = OB.Cells(spec, obs, None, rays_per_block=1)
    structs = attach(p, az4, 5, take=take)
    o = structs['fractions'].objects.contents
    assert o.pad_ == N.OBJ_TRACK | 7 and isinstance(p.ot, N.ObjectsTrack) and (p.ot.max_shift, p.ot.max_pieces, p.ot.shifts_in) == (2, 3, None)
    assert C.addressof(p.ot) == C.addressof(o) == C.addressof(p.o) == C.addressof(p.om)
    plain = OB.Cells(OB.Objects(fr, connectivity=8, max_objects=5, match=True, max_pieces=7), obs, None, rays_per_block=1)
    attach(plain, az4, 5, take=take)
    assert plain.ot is None and plain.o.pad_ == 7
    assert p.arrays() == plain.arrays() + [('track_correlation', u4, (3, 2, 5, 5)), ('track_shift', i4, (3, 2, 2)), ('track_n_pieces', u4, (3, 2)),
                                          ('track_pieces', u4, (3, 2, 3, 10)), ('track_covered', u4, (3, 2, 2, 5))]
    bound = {}
    for i, (path, _, _) in enumerate(p.arrays()):
        bound[path] = 0x1000 * (i + 1)
        p.bind(path, bound[path])
    ot = C.cast(structs['fractions'].objects, C.POINTER(N.ObjectsTrack)).contents
    assert (ot.correlation, ot.shift, ot.n_pieces, ot.pieces, ot.covered) == tuple(bound['track_' + k] for k in ('correlation', 'shift', 'n_pieces', 'pieces', 'covered'))
    assert (ot.m.n_pieces, ot.m.pieces, ot.m.covered, ot.m.o.table) == (bound['n_pieces'], bound['pieces'], bound['covered'], bound['table'])
    # given shifts, no match: no correlation array, the shifts of the call behind the struct, a zero low half of pad_
    g = OB.Cells(OB.Objects(fr, track=True, shifts=[[1, -1], [2, -2]]), obs, None, rays_per_block=2)
    structs = attach(g, az4, 5, take=take)
    assert [a[0] for a in g.arrays()[-4:]] == ['track_shift', 'track_n_pieces', 'track_pieces', 'track_covered'] and g.arrays()[-4][2] == (1, 2, 2)
    assert 'track_correlation' not in [a[0] for a in g.arrays()] and g.om is None and g.o.pad_ == N.OBJ_TRACK and g.ot.max_shift == -1
    assert np.ctypeslib.as_array(C.cast(g.ot.shifts_in, C.POINTER(C.c_int32)), shape=(1, 2, 2)).tolist() == [[[1, -1], [2, -2]]]
    # the refusals of a call: one block, an ensemble call, shifts that do not fit the call
    with pytest.raises(ValueError, match='yields 1 block'):
        attach(OB.Cells(spec, obs, None), az4, 5, take=take)
    with pytest.raises(ValueError, match='members, not times'):
        attach(OB.Cells(spec, obs, None, rays_per_block=4), np.arange(8.0), 5, n_members=2, take=take)
    with pytest.raises(ValueError, match='does not broadcast'):
        attach(OB.Cells(OB.Objects(fr, track=True, shifts=np.zeros((2, 2, 2), i4)), obs, None, rays_per_block=1), az4, 5, take=take)
    # device outputs
    d = OB.Cells(spec, rays_per_block=2)
    attach(d, az4, 5)
    d.bind_device({'values': {'KDP': 5}, 'count': 6, 'observed': 7, 'sums': 9, 'totals': 10, 'n_objects': 11, 'table': 16, 'labels': 13,
                   'n_pieces': 21, 'pieces': 22, 'covered': 23, 'track_correlation': 31, 'track_shift': 32, 'track_n_pieces': 33,
                   'track_pieces': 34, 'track_covered': 35})
    assert (d.ot.correlation, d.ot.shift, d.ot.n_pieces, d.ot.pieces, d.ot.covered, d.om.pieces) == (31, 32, 33, 34, 35, 22)
    e = OB.Cells(OB.Objects(fr, match=True), rays_per_block=2)
    attach(e, az4, 5)
    with pytest.raises(ValueError, match="unknown entry 'track_shift'"):
        e.bind_device({'track_shift': 1})
    # a call that does not finish the pass: no arrays, no struct
    p.phase = 1
    structs = attach(p, az4, 5, take=take)
    assert sorted(structs) == ['composite'] and p.arrays() == [] and p.ot is None
    # the scratch limit counts the track: 30 blocks of 1023 x 1023 at three thresholds pass without it and are refused with it
    big = NB.Fractions(comp(1023, 1023), 'ZH', [1, 2, 3], [0])
    at = lambda s: attach(OB.Cells(s, np.zeros((1023, 1023), f4), rays_per_block=1), np.arange(30.0), 5, take=take)
    at(OB.Objects(big))
    with pytest.raises(ValueError, match='the pieces and the track of 30 blocks need more than 1 GiB'):
        at(OB.Objects(big, track=True, max_shift=1))
    # the finish
    p.phase = 3
    attach(p, az4, 5, take=take)
    views = {path: np.zeros(sh, dt) for path, dt, sh in p.arrays()}
    views['track_shift'] = np.full((3, 2, 2), -3, i4)
    views['track_n_pieces'] = np.arange(6, dtype=u4).reshape(3, 2)
    ob = p.finish(dict(views), None)['objects']
    assert sorted(ob['track']) == TRACK_KEYS and ob['track']['shift'] is views['track_shift'] and ob['track']['n_pieces'].tolist() == [[0, 1], [2, 3], [4, 5]]
    assert ob['track']['correlation'].shape == (3, 2, 5, 5) and ob['track']['pieces'].shape == (3, 2, 3, 10) and ob['track']['covered'].shape == (3, 2, 2, 5)
    views = {path: np.zeros(sh, dt) for path, dt, sh in g.arrays()}
    assert g.finish(dict(views), None)['objects']['track']['correlation'] is None


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_struct_layout_matches_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){',
             'printf("cpol_objects %zu\\n", sizeof(cpol_objects));', 'printf("cpol_objects_match %zu\\n", sizeof(cpol_objects_match));',
             'printf("cpol_objects_track %zu\\n", sizeof(cpol_objects_track));', 'printf("pad %zu\\n", offsetof(cpol_objects_track, m.o.pad_));',
             'printf("bit %d\\n", CPOL_OBJ_TRACK);', 'printf("limits %d %d\\n", CPOL_TRACK_MAX_SHIFT, CPOL_TRACK_MAX_GIVEN);']
    for fname, _ in N.ObjectsTrack._fields_:
        lines.append('printf("t.%s %%zu\\n", offsetof(cpol_objects_track, %s));' % (fname, fname))
    lines.append('cpol_objects_track t; memset(&t, 0, sizeof t); printf("off %d\\n", (t.m.o.pad_ & CPOL_OBJ_TRACK) == 0); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got['cpol_objects']) == C.sizeof(N.Objects) == 96 and int(got['cpol_objects_match']) == C.sizeof(N.ObjectsMatch) == 120
    assert int(got['cpol_objects_track']) == C.sizeof(N.ObjectsTrack) == 176
    for fname, _ in N.ObjectsTrack._fields_:
        assert int(got['t.' + fname]) == getattr(N.ObjectsTrack, fname).offset, fname
    assert [n for n, _ in N.ObjectsTrack._fields_] == ['m', 'max_shift', 'max_pieces', 'shifts_in', 'correlation', 'shift', 'n_pieces', 'pieces', 'covered']
    assert N.ObjectsTrack.m.offset == 0 and int(got['pad']) == 12 and int(got['bit']) == N.OBJ_TRACK == 1 << 30 and got['off'] == '1'
    assert got['limits'] == '%d %d' % (OB.TRACK_MAX_SHIFT, OB.TRACK_MAX_GIVEN) == '32 1023'
    # the struct of a spec: bare without anything, an ObjectsMatch with the match alone, an ObjectsTrack with the track
    f = N.Fractions()
    fr = NB.Fractions(comp(3, 2), 'ZH', [1], [0])
    o, keep = N.Context.objects_struct(OB.Objects(fr), f)
    assert type(keep[0]) is N.Objects and o.pad_ == 0
    o, keep = N.Context.objects_struct(OB.Objects(fr, match=True, max_pieces=9), f)
    assert type(keep[0]) is N.ObjectsMatch and o.pad_ == 9
    o, keep = N.Context.objects_struct(OB.Objects(fr, track=True, max_shift=4, max_track_pieces=6), f)
    assert type(keep[0]) is N.ObjectsTrack and o.pad_ == 1 << 30 and (keep[0].max_shift, keep[0].max_pieces) == (4, 6)
    assert C.addressof(f.objects.contents) == C.addressof(keep[0])
    o, keep = N.Context.objects_struct(OB.Objects(fr, match=True, max_pieces=9, track=True, shifts=[0, 1]), f, np.zeros((1, 1, 2), i4))
    assert o.pad_ == (1 << 30) | 9 and keep[0].max_shift == -1 and keep[0].shifts_in == keep[1].ctypes.data


# ---------------------------------------------------------------------------------------------------- the host header
@pytest.fixture(scope='module')
def exes(tmp_path_factory):
    """(obj_track_check, obj_match_check): both with the sanitizers; the older program must still compile against the grown header."""
    out = []
    for name in ('obj_track_check', 'obj_match_check'):
        path = str(tmp_path_factory.mktemp('objt') / name)
        r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', name + '.cpp'),
                            '-o', path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out.append(path)
    return out


def run(exe, mode, *calls):
    r = subprocess.run([exe, mode] + list(calls), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls)
    return lines


def test_obj_check_refusals_and_sizes(exes):
    exe, old = exes
    bit = 1 << 30
    got = run(exe, 'check', 'blocks=1', 'shift=33', 'shift=-2', 'shift=-1', 'shift=2,given=1', 'shift=-1,given=1,gv=1024', 'shift=-1,given=1,gv=-1024',
              'pieces=0', 'pieces=65536', 'sh=0', 'tn=0', 'tp=0', 'tc=0')
    assert got[0] == 'refused the track needs at least two blocks'
    assert got[1] == got[2] == 'refused max_shift must lie in -1 ... 32'
    assert got[3] == 'refused max_shift == -1 needs shifts_in' and got[4] == 'refused shifts_in belongs to max_shift == -1'
    assert got[5] == got[6] == 'refused a given shift must lie in -1023 ... 1023'
    assert got[7] == got[8] == 'refused max_pieces of the track must lie in 1 ... 65535'
    assert got[9] == got[10] == got[11] == got[12] == 'refused shift, n_pieces, pieces or covered of the track is NULL'
    # pad_: negative values and bits 16 ... 29 are refused as ever; without bit 30 nothing behind the match (or the bare struct) is read
    word = 'refused pad_ (max_pieces of a cpol_objects_match) must lie in 0 ... 65535'
    assert run(exe, 'check', 'pad=-1', 'pad=65536', 'pad=%d' % (bit | 65536), 'pad=%d' % (1 << 29), 'pad=%d' % (bit | 1 << 16), 'pad=%d' % -bit) == [word] * 6
    assert run(exe, 'check', 'pad=0', 'pad=5', 'pad=5,np=0', 'pad=%d,np=0' % (bit | 5)) == [
        'ok scratch 168 track 0 match 0', 'ok scratch 280 track 0 match 1', 'refused n_pieces, pieces or covered is NULL',
        'refused n_pieces, pieces or covered is NULL']
    # nx 3, ny 2, two blocks, one threshold: 3 maps of 14 words; the masks of 2 blocks x 2 rows x 1 word, one piece map
    line, = run(exe, 'check', 'shift=2,pieces=8,max=16')
    assert line == ('ok scratch 256 track 1 match 0 pairs 1 maps 1 side 5 words 1 bits 168 pieceoff 200 piecebytes 56 corroff 256 corrbytes 100 '
                    'bitsgrid 2 corrgrid 1 slabs 1 shiftgrid 1 rows 1 cellgroups 1 decode 1 shiftbytes 8 n 4 pieces 320 covered 128 given 0')
    # a correlation that is computed but not wanted lies in the scratch; given shifts need none
    assert run(exe, 'check', 'shift=2,corr=0')[0].startswith('ok scratch 356 track 1 ')
    line, = run(exe, 'check', 'shift=-1,given=1,gv=-1023,blocks=3,nthr=2')
    assert ' side 1 ' in line and ' corrbytes 0 ' in line and line.endswith(' given 8') and ' pairs 2 maps 4 ' in line
    # the match inside: its piece scratch first, the track's behind it
    line, = run(exe, 'check', 'pad=%d' % (bit | 5))
    assert line.startswith('ok scratch %d track 1 match 1 pairs 1 maps 1 side 5 words 1 bits 280 pieceoff 312 ' % (280 + 32 + 56))
    # the measured case: 12 times, 300 x 300, three thresholds, max_shift 8
    cells, per = 90000, (2 * 90000 + 300) * 4
    line, = run(exe, 'check', 'nx=300,ny=300,blocks=12,nthr=3,shift=8,max=1024,pieces=1024')
    lab, bits = 13 * 3 * per, 12 * 3 * 300 * 5 * 8
    assert line == ('ok scratch %d track 1 match 0 pairs 11 maps 33 side 17 words 5 bits %d pieceoff %d piecebytes %d corroff %d corrbytes %d '
                    'bitsgrid %d corrgrid %d slabs 19 shiftgrid 9 rows %d cellgroups %d decode %d shiftbytes 264 n 132 pieces %d covered %d given 0'
                    % (lab + bits + 33 * per, lab, lab + bits, 33 * per, lab + bits + 33 * per, 33 * 289 * 4, 12 * 75, 33 * 19, 11 * 75,
                       -(-33 * cells // 256), -(-33 * 1024 // 256), 33 * 1024 * 40, 33 * 2 * 1024 * 4))
    spec = OB.Objects(NB.Fractions(comp(300, 300), 'ZH', [1, 2, 3], [0]), track=True, max_shift=8)
    assert OB.scratch_bytes(spec, 12) == lab + bits + 33 * per
    # odd grids: the masks begin on an 8-byte boundary
    assert run(exe, 'check', 'nx=3,ny=3,shift=1')[0].startswith('ok scratch %d track 1 match 0 pairs 1 maps 1 side 3 words 1 bits 256 pieceoff 304 ' % (304 + 84))
    odd = OB.Objects(NB.Fractions(comp(3, 3), 'ZH', [1], [0]), track=True, max_shift=1)
    assert OB.scratch_bytes(odd, 2) == 304 + 84
    # a case that passes without the track and is refused with it
    big = 'nx=1023,ny=1023,blocks=30,nthr=3,max=1'
    assert run(exe, 'check', big + ',pad=0')[0] == 'ok scratch %d track 0 match 0' % (31 * 3 * (2 * 1023 * 1023 + 1023) * 4)
    assert run(exe, 'check', big)[0] == 'refused the scratch with the track\'s masks and piece maps must be at most 1 GiB'
    # the older program prints what it printed
    assert run(old, 'check', 'pieces=0', 'pieces=-1', 'pieces=65536', 'pieces=65535,max=7')[:3] == [
        'ok scratch %d match 0' % (2 * 14 * 4), 'refused pad_ (max_pieces of a cpol_objects_match) must lie in 0 ... 65535',
        'refused pad_ (max_pieces of a cpol_objects_match) must lie in 0 ... 65535']


def test_host_build_of_the_track_against_the_rule(exes, tmp_path):
    """The packing, obj_track_count over slabs, obj_track_key / obj_track_unkey and obj_track_number of cpol_obj.h, single-threaded,
    on the grids of the GPU tests against the rule."""
    exe = exes[0]
    rng = np.random.default_rng(5)
    files, want = [], []

    def case(ke, kl, S, given=(0, 0)):
        corr = OB.correlation_of_pair(ke, kl, S) if S >= 0 else np.zeros(0, u4)
        shift = OB.shift_of(corr) if S >= 0 else given
        overlap = (OB.shift_labels(ke.astype(i4), *shift) > 0) & kl
        path = str(tmp_path / ('case%d.bin' % len(files)))
        with open(path, 'wb') as fh:
            np.array(ke.shape + (S,) + tuple(given), i4).tofile(fh)
            ke.astype(u1).tofile(fh)
            kl.astype(u1).tofile(fh)
            corr.tofile(fh)
            np.array(shift, i4).tofile(fh)
            overlap.astype(u1).tofile(fh)
        files.append(path)
        want.append('ok shift %d %d cells %d' % (shift[0], shift[1], overlap.sum()))
    for n_y in (1, 2, 17, 33):
        for n_x in (1, 2, 63, 64, 65, 129):
            for S in (0, 1, 2, 32):
                ke = rng.random((n_y, n_x)) < 0.4
                case(ke, moved(ke, int(rng.integers(-2, 3)), int(rng.integers(-2, 3))) | (rng.random((n_y, n_x)) < 0.05), S)
            full = np.ones((n_y, n_x), bool)
            case(full, full, 32)
            case(~full, full, 2)
            for given in ((0, 0), (1, -1), (-n_y, 0), (0, n_x), (1023, -1023), (n_y - 1, 1 - n_x)):
                case(full, rng.random((n_y, n_x)) < 0.7, -1, given)
    # an object that crosses the 64-cell boundary only after the shift; ties
    ke = np.zeros((3, 130), bool)
    ke[1, 58:63] = True
    case(ke, moved(ke, 0, 4), 8)
    case(ke, moved(ke, 1, 4) | moved(ke, -1, -4), 8)
    assert want[-2].startswith('ok shift 0 4 ') and want[-1].startswith('ok shift -1 -4 ')
    lines = []
    for at in range(0, len(files), 100):
        lines += run(exe, 'track', *files[at:at + 100])
    assert lines == want
    assert sum(int(l.split()[-1]) > 0 for l in want) > 100
