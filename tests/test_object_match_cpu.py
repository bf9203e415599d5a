"""The match of the object cells without a GPU: the rule (cosmo_pol_amd/objects.py: `pieces_of_map`, `cells` with match) against a
literal flood fill over the overlap map with a dict of cell keys; the host folds `pairs`, `match` and `contingency` against
np.unique of per-cell keys and on hand-made maps with known answers; every ValueError of the spec and the key with match off;
the product object `Cells`; the ctypes mirror of cpol_objects_match against the header; and the host header
(cosmo_pol_amd/csrc/cpol_obj.h) through tests/c_host/obj_match_check.cpp, built with the address and undefined-behaviour
sanitizers and run as a program of its own: the new refusals and sizes of obj_check(), and the match's per-cell functions driven
single-threaded with the run, union and find code over the grids of the GPU tests against the rule.  All comparisons are exact."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import neighbourhood as NB
from cosmo_pol_amd import objects as OB

from _objects import PATTERNS, SHAPES, pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f4, u1, u4, u8, i4, i8 = np.float32, np.uint8, np.uint32, np.uint64, np.int32, np.int64
PIECE_KEYS = ('n_pieces', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'forecast', 'observed')
ATTRS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak', 'peak_cell')


def comp(n_x, n_y):
    return CP.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0))


def spec_of(n_x, n_y, thresholds=(0.5,), **kw):
    kw.setdefault('match', True)
    return OB.Objects(NB.Fractions(comp(n_x, n_y), 'ZH', list(thresholds), [0]), **kw)


def labels_of(binary, connectivity, min_area=1):
    return OB.cells_of_map(binary, np.zeros(binary.shape, f4), connectivity, min_area, 1)[2]


# ---------------------------------------------------------------------------------------------------- the literal rule
def literal_pieces(lf, lo, connectivity, max_pieces, max_objects):
    """The match of one pair of label maps cell by cell: a flood fill over the overlap map from every unvisited cell in raster
    order, the visited cells in a dict keyed by (iy, ix)."""
    n_y, n_x = lf.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    inside = {(y, x): 0 for y in range(n_y) for x in range(n_x) if lf[y, x] > 0 and lo[y, x] > 0}
    pieces, covered, n = np.zeros((max_pieces, OB.WORDS), u4), np.zeros((2, max_objects), u4), 0
    for (y, x) in sorted(inside):
        if lf[y, x] <= max_objects:
            covered[0, lf[y, x] - 1] += 1
        if lo[y, x] <= max_objects:
            covered[1, lo[y, x] - 1] += 1
        if inside[(y, x)]:
            continue
        n += 1
        inside[(y, x)] = n
        todo, mine = [(y, x)], [(y, x)]
        while todo:
            cy, cx = todo.pop()
            for dy, dx in steps:
                q = (cy + dy, cx + dx)
                if inside.get(q, 1) == 0:
                    inside[q] = n
                    todo.append(q)
                    mine.append(q)
        # every piece lies in exactly one object of either side
        assert len({int(lf[c]) for c in mine}) == 1 and len({int(lo[c]) for c in mine}) == 1
        if n <= max_pieces:
            ys, xs = np.array([c[0] for c in mine]), np.array([c[1] for c in mine])
            pieces[n - 1] = [y * n_x + x, len(mine), xs.sum(), ys.sum(), xs.min(), xs.max(), ys.min(), ys.max(), lf[y, x], lo[y, x]]
    return u4(n), pieces, covered, inside


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('min_area', [1, 3])
def test_pieces_against_the_flood_fill(connectivity, min_area):
    rng = np.random.default_rng(31 + connectivity + min_area)
    cases = [(rng.random(shape) < d, rng.random(shape) < d) for shape in [(1, 1), (1, 9), (9, 1), (2, 3), (7, 70), (33, 35)]
             for d in (0.3, 0.59, 0.8, 1.0)]
    cases += [(pattern(a, (13, 70)), pattern(b, (13, 70))) for a, b in itertools.product(PATTERNS, PATTERNS)]
    some = split = 0
    for bf, bo in cases:
        lf, lo = labels_of(bf, connectivity, min_area), labels_of(bo, connectivity, min_area)
        for max_pieces, max_objects in ((3, 2), (4096, 4096)):
            n, pieces, covered = OB.pieces_of_map(lf, lo, connectivity, max_pieces, max_objects)
            wn, wp, wc, _ = literal_pieces(lf, lo, connectivity, max_pieces, max_objects)
            assert n == wn and n.dtype == u4 and pieces.dtype == u4 and covered.dtype == u4
            assert np.array_equal(pieces, wp) and np.array_equal(covered, wc), (bf.shape, max_pieces)
        # the invariants on the last of the two, in which nothing overflows
        cells = int(((lf > 0) & (lo > 0)).sum())
        assert pieces[:, OB.AREA].sum() == covered[0].sum() == covered[1].sum() == cells
        area = np.bincount(lf.reshape(-1), minlength=4097)[1:]
        assert (covered[0] <= area[:4096]).all()
        some += int(n)
        split += int(n) > len({(int(a), int(b)) for a, b in pieces[:int(n), OB.FORECAST:]})
    assert some > 500 and split > 10                    # (pieces were found, and objects met in more than one piece)


def test_cells_with_match_and_pairs_against_unique():
    rng = np.random.default_rng(32)
    pool = np.array([np.nan, -np.inf, np.inf, 0.0, -0.0, 0.5, 1.0, 1.0, 2.0, 3.5], dtype=f4)
    maps, obs = pool[rng.integers(0, len(pool), (3, 12, 70))], pool[rng.integers(0, len(pool), (12, 70))]
    dom = (rng.random((12, 70)) < 0.9).astype(u1)
    for connectivity, min_area in ((4, 1), (8, 1), (4, 3), (8, 3)):
        spec = spec_of(70, 12, [-np.inf, 0.0, 1.0, np.inf], connectivity=connectivity, min_area=min_area, max_objects=512)
        res = OB.cells(spec, maps, obs, dom)
        off = OB.cells(spec_of(70, 12, [-np.inf, 0.0, 1.0, np.inf], connectivity=connectivity, min_area=min_area, max_objects=512, match=False),
                       maps, obs, dom)
        assert sorted(set(res) - set(off)) == ['covered', 'covered_observed', 'pieces'] and sorted(res['pieces']) == sorted(PIECE_KEYS)
        for k in ATTRS + ('labels',):
            assert np.array_equal(res[k], off[k]) and np.array_equal(res['observed'][k], off['observed'][k]), k
        assert res['pieces']['n_pieces'].shape == (3, 4) and res['pieces']['bbox'].shape == (3, 4, 512, 4)
        assert res['covered'].shape == res['covered_observed'].shape == (3, 4, 512) and res['covered'].dtype == u4
        assert 'pieces' not in res['observed'] and res['pieces']['n_pieces'].any()
        for b in range(3):
            for t in range(4):
                lf, lo = res['labels'][b, t], res['observed']['labels'][t]
                wn, wp, wc, _ = literal_pieces(lf, lo, connectivity, 512, 512)
                assert res['pieces']['n_pieces'][b, t] == wn
                got = np.stack([res['pieces'][k][b, t] for k in ('first', 'area', 'sum_x', 'sum_y')] + list(res['pieces']['bbox'][b, t].T) +
                               [res['pieces']['forecast'][b, t], res['pieces']['observed'][b, t]], axis=-1)
                assert np.array_equal(got, wp) and np.array_equal(res['covered'][b, t], wc[0]) and np.array_equal(res['covered_observed'][b, t], wc[1])
                # pairs against np.unique of the per-cell keys
                both = (lf > 0) & (lo > 0)
                key, count = np.unique(lf[both].astype(i8) * (1 << 20) + lo[both], return_counts=True)
                p = OB.pairs(res, b, t)
                assert np.array_equal(p['forecast'], key >> 20) and np.array_equal(p['observed'], key & ((1 << 20) - 1)) and np.array_equal(p['area'], count)
                yy, xx = np.nonzero(both)
                inverse = np.searchsorted(key, lf[both].astype(i8) * (1 << 20) + lo[both])
                assert np.array_equal(p['sum_x'], np.bincount(inverse, weights=xx, minlength=key.size).astype(i8))
                assert np.array_equal(p['sum_y'], np.bincount(inverse, weights=yy, minlength=key.size).astype(i8))
                assert p['pieces'].sum() == wn and all(v.dtype == i8 for v in p.values())


def hand(rows_f, rows_o, **kw):
    """A result of one block from two hand-made maps of 0 / 1 cells."""
    bf, bo = np.array(rows_f, f4), np.array(rows_o, f4)
    return OB.cells(spec_of(bf.shape[1], bf.shape[0], **kw), bf, bo)


def test_match_and_contingency_on_hand_made_maps():
    # forecast: one long object (1) and a single cell (2); observed: two objects under the long one, each covering two cells (a tie),
    # the first of them in TWO pieces of one pair, and a third one alone
    res = hand([[1, 1, 1, 1, 1, 1, 1, 0, 1],
                [0, 0, 0, 0, 0, 0, 0, 0, 0],
                [0, 0, 0, 0, 0, 0, 0, 0, 0]],
               [[1, 0, 1, 0, 1, 1, 0, 0, 0],
                [1, 1, 1, 0, 0, 0, 0, 0, 0],
                [0, 0, 0, 0, 0, 0, 0, 1, 1]], max_objects=4)
    assert res['n_objects'].tolist() == [[2]] and res['observed']['n_objects'].tolist() == [3]
    assert res['pieces']['n_pieces'].tolist() == [[3]]
    assert res['pieces']['forecast'][0, 0].tolist() == [1, 1, 1, 0] and res['pieces']['observed'][0, 0].tolist() == [1, 1, 2, 0]
    assert res['pieces']['area'][0, 0].tolist() == [1, 1, 2, 0] and res['pieces']['bbox'][0, 0, 2].tolist() == [4, 5, 0, 0]
    assert res['covered'][0, 0].tolist() == [4, 0, 0, 0] and res['covered_observed'][0, 0].tolist() == [2, 2, 0, 0]
    p = OB.pairs(res, 0)
    assert (p['forecast'].tolist(), p['observed'].tolist(), p['area'].tolist(), p['pieces'].tolist()) == ([1, 1], [1, 2], [2, 2], [2, 1])
    assert p['sum_x'].tolist() == [0 + 2, 4 + 5] and p['sum_y'].tolist() == [0, 0]
    m = OB.match(res)
    assert m['partner'].tolist() == [[1, 0, 0, 0]] and m['area'].tolist() == [[2, 0, 0, 0]]          # (the tie goes to the smaller number)
    assert m['observed_partner'].tolist() == [[1, 1, 0, 0]] and m['observed_area'].tolist() == [[2, 2, 0, 0]]
    c = OB.contingency(res)
    assert (c['hits'].tolist(), c['misses'].tolist(), c['false_alarms'].tolist()) == ([2], [1], [1])
    assert c['pod'].tolist() == [2 / 3] and c['far'].tolist() == [1 / 3] and c['csi'].tolist() == [0.5]
    # min_cover: observed object 1 has 6 cells of which 2 are covered, object 2 has 2 of 2; the long forecast object 4 of 7
    c = OB.contingency(res, min_cover=0.4)
    assert (c['hits'].tolist(), c['misses'].tolist(), c['false_alarms'].tolist()) == ([1], [2], [1])
    c = OB.contingency(res, min_cover=0.6)
    assert (c['hits'].tolist(), c['misses'].tolist(), c['false_alarms'].tolist()) == ([1], [2], [2])
    # overflowed pieces: true count, truncated rows, complete covered; pairs refuses, match gives -1, contingency stands
    few = hand([[1, 1, 1, 1, 1, 1, 1, 0, 1]], [[1, 0, 1, 0, 1, 1, 0, 0, 0]], max_objects=4, max_pieces=2)
    assert few['pieces']['n_pieces'].tolist() == [[3]] and few['pieces']['first'][0, 0].tolist() == [0, 2]
    assert few['covered'][0, 0].tolist() == [4, 0, 0, 0] and few['covered_observed'][0, 0].tolist() == [1, 1, 2, 0]
    with pytest.raises(ValueError, match='3 pieces, 2 rows'):
        OB.pairs(few, 0)
    m = OB.match(few)
    assert all((m[k] == -1).all() and m[k].shape == (1, 4) for k in m)
    c = OB.contingency(few)
    assert (c['hits'].tolist(), c['misses'].tolist(), c['false_alarms'].tolist()) == ([3], [0], [1])
    # overflowed objects: numbers beyond max_objects are named in the rows, covered holds the rows up to max_objects alone, and the
    # contingency is not silently partial
    over = hand([[1, 0, 1, 0, 1]], [[1, 1, 1, 1, 1]], max_objects=2, max_pieces=8)
    assert over['n_objects'].tolist() == [[3]] and over['pieces']['forecast'][0, 0, :3].tolist() == [1, 2, 3]
    assert over['covered'][0, 0].tolist() == [1, 1] and over['covered_observed'][0, 0].tolist() == [3, 0]
    c = OB.contingency(over)
    assert c['hits'].tolist() == [-1] and np.isnan(c['csi']).all()
    assert OB.match(over)['observed_partner'].tolist() == [[1, 0]]
    # nothing to match, and what the folds refuse
    none = hand([[1, 0]], [[0, 1]])
    assert none['pieces']['n_pieces'].tolist() == [[0]] and OB.pairs(none, 0)['area'].size == 0 and not OB.match(none)['partner'].any()
    c = OB.contingency(none)
    assert (c['hits'].tolist(), c['misses'].tolist(), c['false_alarms'].tolist()) == ([0], [1], [1]) and c['pod'].tolist() == [0.0]
    plain = OB.cells(spec_of(2, 1, match=False), np.ones((1, 2), f4), np.ones((1, 2), f4))
    for fold in (lambda r: OB.pairs(r, 0), OB.match, OB.contingency):
        with pytest.raises(ValueError, match='has no match'):
            fold(plain)
    with pytest.raises(ValueError, match='threshold index outside'):
        OB.match(none, 1)
    with pytest.raises(ValueError, match='min_cover'):
        OB.contingency(none, min_cover=1.0)


def test_spec_refusals_identity_and_key():
    fr = NB.Fractions(comp(4, 3), 'ZH', [0.1, 0.2], [1, 2])
    off, on = OB.Objects(fr), OB.Objects(fr, match=True)
    # with match off the key and the repr are today's
    assert off.key == (fr.key, 4, 1, 1024, True) and (off.match, off.max_pieces) == (False, None) and 'match' not in repr(off)
    assert OB.Objects(fr, sums=True).key == (fr.key, 4, 1, 1024, True, True, None)
    assert (on.match, on.max_pieces) == (True, 1024) and on.key == off.key + ('match', 1024) and repr(on).endswith(', match=True, max_pieces=1024)')
    assert on != off and on == OB.Objects(fr, match=True, max_pieces=1024) and hash(on) == hash(OB.Objects(fr, match=True))
    assert on != OB.Objects(fr, match=True, max_pieces=7) and OB.Objects(fr, max_objects=9, match=True).max_pieces == 9
    both = OB.Objects(fr, sums=True, match=True, max_pieces=5)
    assert both.key == (fr.key, 4, 1, 1024, True, True, None, 'match', 5) and 'sums=True, match=True, max_pieces=5' in repr(both)
    for kw, text in (({'max_pieces': 5}, 'max_pieces: belongs to match=True'), ({'match': True, 'max_pieces': 0}, 'max_pieces must lie in'),
                     ({'match': True, 'max_pieces': 65536}, 'max_pieces must lie in'), ({'match': True, 'max_pieces': 2.0}, 'max_pieces: an integer'),
                     ({'match': True, 'max_pieces': True}, 'max_pieces: an integer')):
        with pytest.raises(ValueError, match=text):
            OB.Objects(fr, **kw)
    # the scratch: the pieces of the blocks alone behind everything else, 8-byte aligned
    assert OB.scratch_bytes(off, 2) == 3 * 2 * (2 * 12 + 3) * 4
    assert OB.scratch_bytes(on, 2) == 3 * 2 * 27 * 4 + 2 * 2 * 27 * 4
    odd = OB.Objects(NB.Fractions(comp(3, 3), 'ZH', [0.1], [0]), match=True)
    assert OB.scratch_bytes(odd, 1) == (2 * 21 * 4 + 7) // 8 * 8 + 21 * 4
    sums = OB.Objects(fr, sums=True, match=True, max_objects=3)
    assert OB.scratch_bytes(sums, 2) == OB.scratch_bytes(OB.Objects(fr, sums=True, max_objects=3), 2) + 2 * 2 * 27 * 4


# ---------------------------------------------------------------------------------------------------- the product object
def attach(product, az, n_gates, n_members=None, take=None):
    structs, keep = product.attach(N, az, n_gates, n_members, True, True, ['U', 'V', 'W', 'T'], take)
    return structs


def test_cells_arrays_binding_finish_join():
    c = CP.Composite(['KDP', 'ZH'], [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0], products=('max', 'lowest'))      # a 2 x 3 grid
    fr = NB.Fractions(c, 'KDP', [0.5, 1.5], [0, 1, 4], plane='lowest')
    spec = OB.Objects(fr, connectivity=8, min_area=2, max_objects=5, match=True, max_pieces=7)
    obs = np.arange(6, dtype=f4).reshape(2, 3)
    p = OB.Cells(spec, obs, None, keep_gates=False, phase=3, rays_per_block=2)

    def take(block):
        return [np.zeros(sh, dt) for _, dt, sh in block], [0x77000 + 64 * i for i in range(len(block))]
    az4 = np.arange(4.0)
    structs = attach(p, az4, 5, take=take)
    f = structs['fractions']
    o = f.objects.contents
    assert (o.connectivity, o.min_area, o.max_objects, o.pad_) == (8, 2, 5, 7) and isinstance(p.om, N.ObjectsMatch)
    assert C.addressof(p.om) == C.addressof(o) == C.addressof(p.o)
    plain = OB.Cells(OB.Objects(fr, connectivity=8, min_area=2, max_objects=5), obs, None, rays_per_block=2)
    attach(plain, az4, 5, take=take)
    assert plain.om is None and plain.o.pad_ == 0
    assert p.arrays() == plain.arrays() + [('n_pieces', u4, (2, 2)), ('pieces', u4, (2, 2, 7, 10)), ('covered', u4, (2, 2, 2, 5))]
    bound = {}
    for i, (path, _, _) in enumerate(p.arrays()):
        bound[path] = 0x1000 * (i + 1)
        p.bind(path, bound[path])
    o = structs['fractions'].objects.contents
    om = C.cast(structs['fractions'].objects, C.POINTER(N.ObjectsMatch)).contents
    assert (o.n_objects, o.table, o.labels) == (bound['n_objects'], bound['table'], bound['labels'])
    assert (om.n_pieces, om.pieces, om.covered) == (bound['n_pieces'], bound['pieces'], bound['covered'])
    # with the exact sums beside it: the match's arrays come last
    q = OB.Cells(OB.Objects(fr, labels=False, sums=True, match=True), obs, None, rays_per_block=4)
    attach(q, az4, 5, n_members=3, take=take)
    assert [a[0] for a in q.arrays()[-9:]] == ['n_objects', 'table', 'volume', 'skipped', 'field', 'field_cells', 'n_pieces', 'pieces', 'covered']
    assert q.arrays()[-1] == ('covered', u4, (3, 2, 2, 1024)) and q.o.sums == 1 and q.o.pad_ == 1024
    # device outputs: the three entries are accepted with match on, and refused as unknown without it
    d = OB.Cells(spec)
    structs = attach(d, az4, 5)
    d.bind_device({'values': {'KDP': 5}, 'count': 6, 'observed': 7, 'sums': 9, 'totals': 10, 'n_objects': 11, 'table': 16, 'labels': 13,
                   'n_pieces': 21, 'pieces': 22, 'covered': 23})
    assert (d.om.n_pieces, d.om.pieces, d.om.covered, d.o.table) == (21, 22, 23, 16)
    e = OB.Cells(OB.Objects(fr))
    attach(e, az4, 5)
    with pytest.raises(ValueError, match="unknown entry 'pieces'"):
        e.bind_device({'pieces': 1})
    # a call that does not finish the pass: no arrays, no struct
    p.phase = 1
    structs = attach(p, az4, 5, take=take)
    assert sorted(structs) == ['composite'] and p.arrays() == [] and p.o is None and p.om is None
    p.bind_device({'pieces': 1, 'nonsense': 2})
    # the scratch limit counts the pieces: 38 blocks pass without the match and are refused with it
    big = NB.Fractions(comp(1023, 1023), 'ZH', [1, 2, 3], [0])
    at = lambda s: attach(OB.Cells(s, np.zeros((1023, 1023), f4), rays_per_block=1), np.arange(38.0), 5, take=take)
    at(OB.Objects(big))
    with pytest.raises(ValueError, match='the labelling scratch, the sums and the pieces of 38 blocks need more than 1 GiB'):
        at(OB.Objects(big, match=True))
    # the finish and the join
    p.phase = 3
    attach(p, az4, 5, take=take)
    views = {path: np.zeros(sh, dt) for path, dt, sh in p.arrays()}
    views['pieces'] = np.arange(10, dtype=u4) * np.ones((2, 2, 7, 10), u4)
    views['n_pieces'] = np.array([[1, 2], [3, 4]], u4)
    views['covered'] = np.arange(2, dtype=u4)[:, None] * np.ones((2, 2, 2, 5), u4) + u4(7)
    out = p.finish(dict(views), None)
    ob = out['objects']
    assert sorted(ob) == sorted(ATTRS + ('labels', 'observed', 'connectivity', 'min_area', 'thresholds', 'pieces', 'covered', 'covered_observed'))
    pc = ob['pieces']
    assert sorted(pc) == sorted(PIECE_KEYS) and pc['n_pieces'].tolist() == [[1, 2], [3, 4]] and (pc['area'] == 1).all()
    assert pc['bbox'].shape == (2, 2, 7, 4) and (pc['bbox'] == [4, 5, 6, 7]).all() and (pc['forecast'] == 8).all() and (pc['observed'] == 9).all()
    assert ob['covered'].shape == (2, 2, 5) and (ob['covered'] == 7).all() and (ob['covered_observed'] == 8).all()
    j = p.join([out, out], np.concatenate)['objects']
    assert j['pieces']['n_pieces'].shape == (4, 2) and j['pieces']['bbox'].shape == (4, 2, 7, 4) and j['covered'].shape == (4, 2, 5)
    assert j['covered_observed'].shape == (4, 2, 5) and j['observed'] is ob['observed'] and j['n_objects'].shape == (4, 2)
    p.rays_per_block = 0
    assert p.join([None, out], np.concatenate)['objects'] is ob


def test_cells_block_through_the_packer():
    class Pool(object):
        def take(self, nbytes, writer=None):
            return np.zeros(nbytes + 64, np.uint8), {'ctx': None, 'serial': 0}
    p = OB.Cells(spec_of(3, 2, max_objects=3, max_pieces=2), np.arange(6, dtype=f4).reshape(2, 3))
    attach(p, np.arange(4.0), 5, take=lambda block: N.carve_block(Pool(), block)[:2])
    views, addresses, _ = N.carve_block(Pool(), p.arrays())
    assert [v.shape for v in views[-3:]] == [(1, 1), (1, 1, 2, 10), (1, 1, 2, 3)] and all((a - addresses[0]) % 64 == 0 for a in addresses)


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_struct_layout_matches_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){',
             'printf("cpol_objects %zu\\n", sizeof(cpol_objects));', 'printf("cpol_objects_match %zu\\n", sizeof(cpol_objects_match));',
             'printf("pad %zu\\n", offsetof(cpol_objects_match, o.pad_));']
    for fname, _ in N.ObjectsMatch._fields_:
        lines.append('printf("m.%s %%zu\\n", offsetof(cpol_objects_match, %s));' % (fname, fname))
    lines.append('cpol_objects_match m; memset(&m, 0, sizeof m); printf("off %d\\n", m.o.pad_ == 0); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got['cpol_objects']) == C.sizeof(N.Objects) == 96 and int(got['cpol_objects_match']) == C.sizeof(N.ObjectsMatch) == 120
    for fname, _ in N.ObjectsMatch._fields_:
        assert int(got['m.' + fname]) == getattr(N.ObjectsMatch, fname).offset, fname
    assert [n for n, _ in N.ObjectsMatch._fields_] == ['o', 'n_pieces', 'pieces', 'covered'] and N.ObjectsMatch.o.offset == 0
    assert int(got['pad']) == N.Objects.pad_.offset == 12 and got['off'] == '1' and N.ObjectsMatch().o.pad_ == 0
    # Objects keeps its fields; the struct of a spec without match is a bare Objects with a zero pad_
    assert [n for n, _ in N.Objects._fields_][:4] == ['connectivity', 'min_area', 'max_objects', 'pad_'] and len(N.Objects._fields_) == 15
    f = N.Fractions()
    o, keep = N.Context.objects_struct(OB.Objects(NB.Fractions(comp(3, 2), 'ZH', [1], [0])), f)
    assert type(keep[0]) is N.Objects and o.pad_ == 0 and C.addressof(f.objects.contents) == C.addressof(o)
    o, keep = N.Context.objects_struct(spec_of(3, 2, max_pieces=9), f)
    assert type(keep[0]) is N.ObjectsMatch and o.pad_ == 9 and C.addressof(f.objects.contents) == C.addressof(keep[0])


# ---------------------------------------------------------------------------------------------------- the host header
@pytest.fixture(scope='module')
def exes(tmp_path_factory):
    """(obj_match_check, obj_check): both with the sanitizers; the older program must still compile against the grown header."""
    out = []
    for name in ('obj_match_check', 'obj_check'):
        path = str(tmp_path_factory.mktemp('objm') / name)
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
    got = run(exe, 'check', 'pieces=0', 'pieces=-1', 'pieces=65536', 'pieces=5,np=0', 'pieces=5,pc=0', 'pieces=5,cov=0', 'pieces=65535,max=7',
              'pieces=5,conn=5', 'pieces=5,sums=1,weight=1')
    assert got[0] == 'ok scratch %d match 0' % (2 * 14 * 4)             # (a bare cpol_objects of 96 bytes: nothing behind it is read)
    assert got[1] == got[2] == 'refused pad_ (max_pieces of a cpol_objects_match) must lie in 0 ... 65535'
    assert got[3] == got[4] == got[5] == 'refused n_pieces, pieces or covered is NULL'
    # nx 3, ny 2, one block, one threshold: 2 maps of (2 * 6 + 2) words, then the one piece map
    assert got[6] == ('ok scratch %d match 1 maxpieces 65535 piecemaps 1 offset 112 piecebytes 56 rows 1 cellgroups 1 decode 256 n 4 '
                      'pieces %d covered 56' % (112 + 56, 65535 * 40))
    assert got[7] == 'refused connectivity must be 4 or 8' and got[8] == 'refused a weight table needs 2 ... 1024 breakpoints'
    # the measured case: 21 members and the observation, 300 x 300, three thresholds; the pieces behind the labelling scratch, and
    # with the exact sums and a weight table behind those, whose offsets do not move
    maps, pm, cells = 22 * 3, 21 * 3, 90000
    lab = maps * (2 * cells + 300) * 4
    line, = run(exe, 'check', 'nx=300,ny=300,blocks=21,nthr=3,conn=8,area=4,max=1024,labels=1,pieces=2048')
    assert line == ('ok scratch %d match 1 maxpieces 2048 piecemaps %d offset %d piecebytes %d rows %d cellgroups %d decode %d n %d pieces %d '
                    'covered %d' % (lab + pm * (2 * cells + 300) * 4, pm, lab, pm * (2 * cells + 300) * 4, 21 * 75, -(-pm * cells // 256),
                                    -(-pm * 2048 // 256), pm * 4, pm * 2048 * 40, pm * 2 * 1024 * 4))
    spec = OB.Objects(NB.Fractions(comp(300, 300), 'ZH', [1, 2, 3], [0]), match=True, max_pieces=2048)
    assert OB.scratch_bytes(spec, 21) == lab + pm * (2 * cells + 300) * 4 == 47_599_200 + 45_435_600
    plain, = run(exe, 'check', 'nx=300,ny=300,blocks=21,nthr=3,max=1024,sums=1,weight=241')
    with_match, = run(exe, 'check', 'nx=300,ny=300,blocks=21,nthr=3,max=1024,sums=1,weight=241,pieces=1024')
    wspec = OB.Objects(spec.fractions, sums=True, weight=OB.zr_table(), match=True)
    before = OB.scratch_bytes(OB.Objects(spec.fractions, sums=True, weight=OB.zr_table()), 21)
    assert len(wspec.weight[0]) == 241 and plain == 'ok scratch %d match 0' % before
    assert with_match.startswith('ok scratch %d match 1 maxpieces 1024 piecemaps 63 offset %d ' % (OB.scratch_bytes(wspec, 21), (before + 7) // 8 * 8))
    # odd grids: the piece scratch begins on an 8-byte boundary
    assert run(exe, 'check', 'nx=3,ny=3,pieces=4')[0].startswith('ok scratch %d match 1 maxpieces 4 piecemaps 1 offset 168 piecebytes 84 ' % (168 + 84))
    # a case that passes without the match and is refused with it: 39 sources x 3 thresholds of 1023 x 1023
    big = 'nx=1023,ny=1023,blocks=38,nthr=3,max=1'
    assert run(exe, 'check', big)[0] == 'ok scratch %d match 0' % (39 * 3 * (2 * 1023 * 1023 + 1023) * 4)
    assert run(exe, 'check', big + ',pieces=1')[0] == 'refused the labelling scratch, the sums\' accumulators and the piece scratch must be at most 1 GiB'
    assert OB.scratch_bytes(OB.Objects(NB.Fractions(comp(1023, 1023), 'ZH', [1, 2, 3], [0]), match=True), 38) > OB.MAX_SCRATCH_BYTES
    # the older program prints what it printed
    assert run(old, 'check', 'nx=7,ny=5,max=65535,nthr=4')[0] == 'ok maps 8 cells 35 scratch %d rows 4 cellgroups 2 decode 2048 n 32 table %d labels 0' % (
        8 * 75 * 4, 8 * 65535 * 40)
    assert run(old, 'check', 'obj=0', 'conn=5') == ['off', 'refused connectivity must be 4 or 8']


def test_host_build_of_the_match_against_the_rule(exes, tmp_path):
    """obj_match_flag, obj_match_cover and the run, union and find code of cpol_obj.h, single-threaded, over pairs of the patterns
    and random maps on the grids of the GPU tests."""
    exe = exes[0]
    rng = np.random.default_rng(33)
    files, want = [], []

    def case(bf, bo, connectivity, min_area, max_pieces=4096, max_objects=4096):
        lf, lo = labels_of(bf, connectivity, min_area), labels_of(bo, connectivity, min_area)
        n, pieces, covered = OB.pieces_of_map(lf, lo, connectivity, max_pieces, max_objects)
        path = str(tmp_path / ('case%d.bin' % len(files)))
        with open(path, 'wb') as fh:
            np.array(bf.shape + (connectivity, min_area, max_pieces, max_objects), i4).tofile(fh)
            bf.astype(u1).tofile(fh)
            bo.astype(u1).tofile(fh)
            lf.astype(i4).tofile(fh)
            lo.astype(i4).tofile(fh)
            np.array([n], u4).tofile(fh)
            pieces.tofile(fh)
            covered.tofile(fh)
        files.append(path)
        want.append((int(n), len(OB._runs((lf > 0) & (lo > 0))[0])))
    pairs = list(itertools.product(PATTERNS, PATTERNS))
    k = 0
    for shape in SHAPES + [(257, 259)]:
        for connectivity, density in ((4, 0.7), (8, 0.6)):
            for min_area in (1, 3):
                case(rng.random(shape) < density, rng.random(shape) < density, connectivity, min_area)
                for _ in range(8):                          # the 64 pairs cycle through the shapes, connectivities and areas
                    a, b = pairs[k % len(pairs)]
                    case(pattern(a, shape), pattern(b, shape), connectivity, min_area)
                    k += 1
    assert k >= 4 * len(pairs)
    # tables that overflow: true count, truncated rows, covered up to max_objects
    board, full = pattern('checkerboard', (65, 67)), pattern('full', (65, 67))
    case(board, full, 4, 1, max_pieces=100, max_objects=50)
    case(full, board, 4, 1, max_pieces=5000, max_objects=50)
    assert want[-1] == (2178, 2178)
    case(np.zeros((1, 1), bool), np.ones((1, 1), bool), 4, 1)
    case(np.ones((1, 1), bool), np.ones((1, 1), bool), 8, 1)
    lines = []
    for at in range(0, len(files), 100):
        lines += run(exe, 'match', *files[at:at + 100])
    for line, (n, runs) in zip(lines, want):
        assert line == 'ok pieces %d runs %d' % (n, runs)
    assert sum(r > n for n, r in want) > 50             # (merges happened: more runs of the overlap map than pieces)
