"""Object cells without a GPU: the rule (cosmo_pol_amd/objects.py: `label`, `cells`) against a literal flood fill and, where
SciPy is installed, against scipy.ndimage.label; the host helpers on hand-made cases; every ValueError of the spec; the product
object `Cells` as tests/test_neighbourhood_cpu.py checks `Scores`; the ctypes mirrors of cpol_objects and the grown
cpol_fractions against the header; and the host header (cosmo_pol_amd/csrc/cpol_obj.h) through tests/c_host/obj_check.cpp, built
with the address and undefined-behaviour sanitizers and run as a program of its own: the refusals and sizes of obj_check(), and
the run, union and find code driven single-threaded over the grids of the GPU tests against the rule's labels.  All comparisons
are exact."""
import ctypes as C
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
f4, u1, u4, u8, i4 = np.float32, np.uint8, np.uint32, np.uint64, np.int32
nan, inf = np.nan, np.inf
ATTRS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak', 'peak_cell')


def comp(n_x, n_y, fields=('ZH',), **kw):
    return CP.Composite(list(fields), np.arange(n_x + 1.0), np.arange(n_y + 1.0), **kw)


def spec_of(n_x, n_y, thresholds, **kw):
    return OB.Objects(NB.Fractions(comp(n_x, n_y), 'ZH', thresholds, [0]), **kw)


# ---------------------------------------------------------------------------------------------------- the literal flood fill
def flood(binary, connectivity):
    """Labels by a literal flood fill from every unlabelled set cell in raster order."""
    n_y, n_x = binary.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    lab = np.zeros((n_y, n_x), dtype=i4)
    n = 0
    for y in range(n_y):
        for x in range(n_x):
            if not binary[y, x] or lab[y, x]:
                continue
            n += 1
            lab[y, x] = n
            todo = [(y, x)]
            while todo:
                cy, cx = todo.pop()
                for dy, dx in steps:
                    yy, xx = cy + dy, cx + dx
                    if 0 <= yy < n_y and 0 <= xx < n_x and binary[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = n
                        todo.append((yy, xx))
    return lab, n


def literal_cells(binary, values, connectivity, min_area, max_objects):
    """The rule for one map, cell by cell in Python."""
    lab, n = flood(binary, connectivity)
    kept, out, table = 0, np.zeros_like(lab), np.zeros((max_objects, OB.WORDS), dtype=u4)
    n_x = binary.shape[1]
    for k in range(1, n + 1):
        ys, xs = np.nonzero(lab == k)
        if len(ys) < min_area:
            continue
        kept += 1
        out[lab == k] = kept
        if kept > max_objects:
            continue
        best = None
        for y, x in zip(ys, xs):                            # raster order: the first of equal peaks stands
            bits = int(np.array(values[y, x], f4).view(u4))
            order = (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits | 0x80000000
            if best is None or order > best[0]:
                best = (order, y * n_x + x, bits)
        table[kept - 1] = [ys[0] * n_x + xs[0], len(ys), xs.sum(), ys.sum(), xs.min(), xs.max(), ys.min(), ys.max(), best[1], best[2]]
    return u4(kept), table, out


@pytest.mark.parametrize('connectivity', [4, 8])
def test_label_against_the_flood_fill(connectivity):
    rng = np.random.default_rng(11)
    for shape in [(1, 1), (1, 9), (9, 1), (2, 3), (7, 70), (70, 7), (33, 35)]:
        for density in (0.0, 0.3, 0.41, 0.59, 0.8, 1.0):
            b = rng.random(shape) < density
            lab, n = OB.label(b, connectivity)
            want, n_want = flood(b, connectivity)
            assert n == n_want and lab.dtype == i4 and np.array_equal(lab, want), (shape, density)
    for name in PATTERNS:
        b = pattern(name, (13, 70))
        lab, n = OB.label(b, connectivity)
        want, n_want = flood(b, connectivity)
        assert n == n_want and np.array_equal(lab, want), name
    with pytest.raises(ValueError, match='2-D bool'):
        OB.label(np.zeros((2, 2), u1))
    with pytest.raises(ValueError, match='connectivity'):
        OB.label(np.zeros((2, 2), bool), 6)


def test_label_against_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(12)
    elements = {4: None, 8: np.ones((3, 3), dtype=int)}
    for connectivity, density in ((4, 0.59), (8, 0.41)):
        for shape in [(65, 67), (130, 5), (5, 130), (257, 259), (1, 1023), (1023, 1)]:
            b = rng.random(shape) < density
            lab, n = OB.label(b, connectivity)
            want, n_want = ndimage.label(b, structure=elements[connectivity])
            assert n == n_want and np.array_equal(lab, want), (connectivity, shape)
        for name in PATTERNS:
            b = pattern(name, (65, 67))
            lab, n = OB.label(b, connectivity)
            want, n_want = ndimage.label(b, structure=elements[connectivity])
            assert n == n_want and np.array_equal(lab, want), (connectivity, name)


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('min_area', [1, 2, 5])
def test_cells_against_the_literal_rule(connectivity, min_area):
    rng = np.random.default_rng(13)
    pool = np.array([nan, -inf, inf, 0.0, -0.0, 0.5, 1.0, 1.0, 2.0, 3.5, 3.5, 1e-42], dtype=f4)
    maps = pool[rng.integers(0, len(pool), (2, 9, 11))]
    obs = pool[rng.integers(0, len(pool), (9, 11))]
    dom = (rng.random((9, 11)) < 0.85).astype(u1)
    spec = spec_of(11, 9, [-inf, 0.0, 1.0, inf], connectivity=connectivity, min_area=min_area, max_objects=6)
    for domain in (None, dom):
        res = OB.cells(spec, maps, obs, domain)
        F, O, m, o = OB.binary_maps(spec.fractions, maps, obs, domain)
        assert sorted(res) == sorted(ATTRS + ('labels', 'observed', 'connectivity', 'min_area', 'thresholds'))
        assert (res['connectivity'], res['min_area']) == (connectivity, min_area) and res['thresholds'] is spec.thresholds
        some = 0
        for s in range(3):
            for t in range(4):
                n, table, lab = literal_cells(F[s, t] if s < 2 else O[t], m[s] if s < 2 else o, connectivity, min_area, 6)
                part = (lambda k: res[k][s, t]) if s < 2 else (lambda k: res['observed'][k][t])
                assert part('n_objects') == n and part('n_objects').dtype == u4 and np.array_equal(part('labels'), lab), (s, t)
                got = np.stack([part('first'), part('area'), part('sum_x'), part('sum_y')] + list(part('bbox').T) +
                               [part('peak_cell'), part('peak').view(u4)], axis=-1)
                assert np.array_equal(got, table), (s, t)
                assert part('peak').dtype == f4 and part('labels').dtype == i4
                some += int(n)
        assert some > 5
    # the table overflowed somewhere (true counts, complete labels), and without labels the key is absent
    res = OB.cells(spec_of(11, 9, [2.0], connectivity=4, max_objects=2, labels=False), maps, obs)
    assert 'labels' not in res and 'labels' not in res['observed'] and res['n_objects'].max() > 2 and res['first'].shape == (2, 1, 2)


def test_peak_order_and_ties():
    # -0.0 lies before +0.0: the peak is +0.0 wherever it lies; equal bits: the smallest flat index
    spec = spec_of(4, 1, [-1.0])
    res = OB.cells(spec, np.array([[-0.0, 0.0, -0.0, 0.0]], f4), np.array([[0.0, -0.0, -0.0, -0.0]], f4))
    assert res['peak_cell'][0, 0, 0] == 1 and res['peak'][0, 0, 0].view(u4) == 0
    assert res['observed']['peak_cell'][0, 0] == 0 and res['observed']['peak'][0, 0].view(u4) == 0
    res = OB.cells(spec, np.array([[-0.0, -0.0, -0.5, -0.0]], f4), np.array([[2.0, 7.0, 7.0, 1.0]], f4))
    assert res['peak_cell'][0, 0, 0] == 0 and res['peak'][0, 0, 0].view(u4) == 0x80000000
    assert res['observed']['peak_cell'][0, 0] == 1 and res['observed']['peak'][0, 0] == 7.0
    assert list(OB.float_order(np.array([-inf, -1.0, -0.0, 0.0, 1e-45, 1.0, inf], f4))) == sorted(
        OB.float_order(np.array([-inf, -1.0, -0.0, 0.0, 1e-45, 1.0, inf], f4)))


def test_host_helpers():
    spec = spec_of(5, 3, [1.0], max_objects=4)
    m = np.array([[1, 1, 0, 0, 5], [1, 0, 0, 0, 5], [0, 0, 3, 0, 5]], f4)
    res = OB.cells(spec, m, np.zeros((3, 5), f4))
    assert list(res['n_objects'][0]) == [3] and list(res['area'][0, 0]) == [3, 3, 1, 0]
    c = OB.centroids(res)
    assert c.shape == (1, 1, 4, 2) and np.allclose(c[0, 0, :3], [[1 / 3 + 0.5, 1 / 3 + 0.5], [4.5, 1.5], [2.5, 2.5]])
    assert np.isnan(c[0, 0, 3]).all() and np.isnan(OB.centroids(res['observed'])).all()
    d = OB.size_distribution(res, [1, 2, 4, 8])
    assert d.shape == (1, 1, 3) and list(d[0, 0]) == [1, 2, 0] and list(OB.size_distribution(res['observed'], [1, 2])[0]) == [0]
    with pytest.raises(ValueError, match='strictly ascending'):
        OB.size_distribution(res, [2, 2])
    assert list(res['bbox'][0, 0, 0]) == [0, 1, 0, 1] and list(res['bbox'][0, 0, 1]) == [4, 4, 0, 2]


def test_spec_refusals_and_identity():
    fr = NB.Fractions(comp(4, 3), 'ZH', [0.1], [1, 2])
    a = OB.Objects(fr)
    assert (a.connectivity, a.min_area, a.max_objects, a.labels) == (4, 1, 1024, True) and a.fractions is fr
    assert a == OB.Objects(fr) and hash(a) == hash(OB.Objects(fr)) and a != OB.Objects(fr, connectivity=8) and a != fr
    assert a != OB.Objects(fr, labels=False) and repr(a).startswith('Objects(Fractions(') and 'connectivity=4' in repr(a)
    assert a.composite is fr.composite and a.thresholds is fr.thresholds and (a.n_x, a.n_y) == (4, 3)
    assert OB.scratch_bytes(a, 2) == 3 * 1 * (2 * 12 + 3) * 4
    for kw, text in (({'connectivity': 6}, 'connectivity must be 4 or 8'), ({'min_area': 0}, 'min_area must be at least 1'),
                     ({'max_objects': 0}, 'max_objects must lie in'), ({'max_objects': 65536}, 'max_objects must lie in'),
                     ({'connectivity': 4.0}, 'connectivity: an integer'), ({'min_area': True}, 'min_area: an integer')):
        with pytest.raises(ValueError, match=text):
            OB.Objects(fr, **kw)
    with pytest.raises(ValueError, match='fractions: a cosmo_pol_amd.neighbourhood.Fractions'):
        OB.Objects(fr.composite)
    # Fractions itself is unchanged
    assert fr.key == (fr.composite.key, 'ZH', 'max', fr.thresholds.tobytes(), fr.radii.tobytes()) and repr(fr).startswith('Fractions(ZH max of')


# ---------------------------------------------------------------------------------------------------- the product object
def attach(product, az, n_gates, n_members=None, take=None):
    structs, keep = product.attach(N, az, n_gates, n_members, True, True, ['U', 'V', 'W', 'T'], take)
    for slot in structs:
        assert slot in dict(N.Outputs._fields_)
    return structs


def test_cells_arrays_binding_finish_join():
    c = CP.Composite(['KDP', 'ZH'], [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0], products=('max', 'lowest'))      # a 2 x 3 grid
    fr = NB.Fractions(c, 'KDP', [0.5, 1.5], [0, 1, 4], plane='lowest')
    spec = OB.Objects(fr, connectivity=8, min_area=2, max_objects=5)
    obs = np.arange(6, dtype=f4).reshape(2, 3)
    dom = np.array([[1, 0, 1], [1, 1, 0]], u1)
    p = OB.Cells(spec, obs, dom, keep_gates=False, phase=3, rays_per_block=2)
    assert (p.name, p.gates, p.spectrum, p.model_var) == ('composite', False, True, None) and p.refuses is CP.Maps.refuses
    assert OB.Cells(spec, obs, keep_gates=True).gates and isinstance(p.scores, NB.Scores) and p.maps is p.scores.maps

    def take(block):
        return [np.zeros(sh, dt) for _, dt, sh in block], [0x77000 + 64 * i for i in range(len(block))]
    az4 = np.arange(4.0)
    structs = attach(p, az4, 5, take=take)
    assert sorted(structs) == ['composite', 'fractions']            # (the cells hang on the fractions: no slot of their own)
    f = structs['fractions']
    o = f.objects.contents
    assert (o.connectivity, o.min_area, o.max_objects) == (8, 2, 5) and (f.n_thresholds, f.n_radii, f.observed) == (2, 3, 0x77000)
    assert p.arrays() == [('ZH', f4, (2, 4, 2, 3)), ('KDP', f4, (2, 4, 2, 3)), ('count', u8, (2, 2, 2, 3)),
                          ('sums', u8, (2, 2, 3, 3)), ('totals', u8, (2, 2, 3)), ('n_objects', u4, (3, 2)),
                          ('table', u4, (3, 2, 5, 10)), ('labels', i4, (3, 2, 2, 3))]
    bound = {}
    for i, (path, _, _) in enumerate(p.arrays()):
        bound[path] = 0x1000 * (i + 1)
        p.bind(path, bound[path])
    o = structs['fractions'].objects.contents
    assert (o.n_objects, o.table, o.labels) == (bound['n_objects'], bound['table'], bound['labels'])
    assert (f.sums, f.totals, structs['composite'].count) == (bound['sums'], bound['totals'], bound['count'])
    # without labels: no array, the slot NULL; an ensemble call: a block per member and the observation
    q = OB.Cells(OB.Objects(fr, labels=False), obs, None, rays_per_block=4)
    f = attach(q, az4, 5, n_members=3, take=take)['fractions']
    assert q.arrays()[-2:] == [('n_objects', u4, (4, 2)), ('table', u4, (4, 2, 1024, 10))] and not f.objects.contents.labels
    # device outputs: the scores' entries and the three of the cells are accepted, any other refused
    d = OB.Cells(spec)
    structs = attach(d, az4, 5)
    f = structs['fractions']
    d.bind_device({'values': {'KDP': 5}, 'count': 6, 'observed': 7, 'sums': 9, 'totals': 10, 'n_objects': 11, 'table': 16, 'labels': 13})
    o = f.objects.contents
    assert (f.observed, f.sums, f.totals, structs['composite'].count) == (7, 9, 10, 6) and (o.n_objects, o.table, o.labels) == (11, 16, 13)
    with pytest.raises(ValueError, match="unknown entry 'ZH'"):
        d.bind_device({'ZH': 1})
    # a call that does not finish the pass: the composite's struct alone, no arrays
    p.phase = 1
    structs = attach(p, az4, 5, take=take)
    assert sorted(structs) == ['composite'] and p.arrays() == [] and p.o is None
    p.bind_device({'table': 1, 'nonsense': 2})
    # what the constructor and the attach refuse
    with pytest.raises(ValueError, match='spec: a cosmo_pol_amd.objects.Objects'):
        OB.Cells(fr, obs)
    with pytest.raises(NotImplementedError, match='process group'):
        OB.Cells(spec, obs, distributed=True)
    big = OB.Objects(NB.Fractions(comp(1023, 1023), 'ZH', [1, 2], [0]))
    with pytest.raises(ValueError, match='labelling scratch of 64 blocks needs more than 1 GiB'):
        attach(OB.Cells(big, np.zeros((1023, 1023), f4), rays_per_block=1), np.arange(64.0), 5, take=take)
    # the finish: the scores' result with one more key; the join: blocks on the leading axis, the observation's cells once
    p.phase = 3
    attach(p, az4, 5, take=take)
    views = {path: np.zeros(sh, dt) for path, dt, sh in p.arrays()}
    views['table'] = np.arange(10, dtype=u4) * np.ones((3, 2, 5, 10), u4)
    views['n_objects'] = np.array([[1, 2], [3, 4], [5, 6]], u4)
    out = p.finish(views, None)
    assert sorted(out) == ['count', 'fractions', 'objects', 'values', 'x_edges', 'y_edges']
    ob = out['objects']
    assert sorted(ob) == sorted(ATTRS + ('labels', 'observed', 'connectivity', 'min_area', 'thresholds'))
    assert ob['n_objects'].tolist() == [[1, 2], [3, 4]] and ob['observed']['n_objects'].tolist() == [5, 6]
    assert ob['area'].shape == (2, 2, 5) and (ob['area'] == 1).all() and ob['bbox'].shape == (2, 2, 5, 4) and (ob['bbox'] == [4, 5, 6, 7]).all()
    assert (ob['peak_cell'] == 8).all() and ob['peak'].dtype == f4 and (ob['peak'].view(u4) == 9).all() and ob['labels'].shape == (2, 2, 2, 3)
    assert ob['observed']['first'].shape == (2, 5) and ob['observed']['labels'].shape == (2, 2, 3)
    j = p.join([out, out], np.concatenate)
    assert j['objects']['n_objects'].shape == (4, 2) and j['objects']['bbox'].shape == (4, 2, 5, 4) and j['objects']['labels'].shape == (4, 2, 2, 3)
    assert j['objects']['observed'] is ob['observed'] and j['objects']['thresholds'] is fr.thresholds and j['fractions']['diff2'].shape == (4, 2, 3)
    p.rays_per_block = 0
    assert p.join([None, out], np.concatenate)['objects'] is ob


def test_cells_block_through_the_packer():
    """The cells' arrays through the operator's own block packer: the table 8-byte aligned (64-byte aligned arrays)."""
    class Pool(object):
        def take(self, nbytes, writer=None):
            return np.zeros(nbytes + 64, np.uint8), {'ctx': None, 'serial': 0}
    spec = spec_of(3, 2, [0.5], max_objects=3)
    p = OB.Cells(spec, np.arange(6, dtype=f4).reshape(2, 3))
    attach(p, np.arange(4.0), 5, take=lambda block: N.carve_block(Pool(), block)[:2])
    views, addresses, _ = N.carve_block(Pool(), p.arrays())
    assert [v.shape for v in views[-3:]] == [(2, 1), (2, 1, 3, 10), (2, 1, 2, 3)] and all((a - addresses[0]) % 64 == 0 for a in addresses)


def test_entry_points_take_objects_or_fractions_alone():
    from cosmo_pol_amd.radar_operator import RadarOperator
    op = RadarOperator.__new__(RadarOperator)
    op.distributed = False
    fr = NB.Fractions(comp(3, 2), 'ZH', [0.5], [0])
    obs = np.zeros((2, 3), f4)
    assert isinstance(op._fss_product(fr, obs, None, None, False, 3, 0), NB.Scores)
    p = op._fss_product(OB.Objects(fr, connectivity=8), obs, None, None, False, 3, 0)
    assert isinstance(p, OB.Cells) and p.spec.connectivity == 8 and p.scores.observed is not None
    for bad in (fr.composite, 'x', None):
        with pytest.raises(ValueError, match='spec: a cosmo_pol_amd.neighbourhood.Fractions, got'):
            op._fss_product(bad, obs, None, None, False, 3, 0)
        with pytest.raises(ValueError, match='spec: a cosmo_pol_amd.neighbourhood.Fractions, got'):
            op.get_network_composite_fss([(0, 0, 0)], [1.0], bad, obs)
    with pytest.raises(ValueError, match='observed: float32'):
        op._fss_product(OB.Objects(fr), np.zeros((3, 3), f4), None, None, False, 3, 0)


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_struct_layout_matches_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){',
             'printf("cpol_objects %zu\\n", sizeof(cpol_objects));', 'printf("cpol_fractions %zu\\n", sizeof(cpol_fractions));']
    for fname, _ in N.Objects._fields_:
        lines.append('printf("o.%s %%zu\\n", offsetof(cpol_objects, %s));' % (fname, fname))
    for fname, _ in N.Fractions._fields_:
        lines.append('printf("f.%s %%zu\\n", offsetof(cpol_fractions, %s));' % (fname, fname))
    lines.append('printf("limits %d %d\\n", CPOL_OBJ_WORDS, CPOL_OBJ_MAX_OBJECTS);')
    lines.append('cpol_fractions f; memset(&f, 0, sizeof f); printf("off %d\\n", f.objects == NULL); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got['cpol_objects']) == C.sizeof(N.Objects) and int(got['cpol_fractions']) == C.sizeof(N.Fractions)
    for fname, _ in N.Objects._fields_:
        assert int(got['o.' + fname]) == getattr(N.Objects, fname).offset, fname
    for fname, _ in N.Fractions._fields_:
        assert int(got['f.' + fname]) == getattr(N.Fractions, fname).offset, fname
    # the new member is the LAST one of cpol_fractions, and a zero struct means off
    assert N.Fractions._fields_[-1][0] == 'objects' and N.Fractions.objects.offset + 8 == C.sizeof(N.Fractions)
    assert got['off'] == '1' and not N.Fractions().objects
    assert got['limits'].split() == [str(OB.WORDS), str(OB.MAX_OBJECTS)] and N.OBJ_WORDS == OB.WORDS
    assert (OB.FIRST, OB.AREA, OB.SUM_X, OB.SUM_Y, OB.X0, OB.X1, OB.Y0, OB.Y1, OB.PEAK_CELL, OB.PEAK_BITS) == tuple(range(10))


# ---------------------------------------------------------------------------------------------------- the host header
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('obj') / 'obj_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'obj_check.cpp'),
                        '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def run(exe, mode, *calls):
    r = subprocess.run([exe, mode] + list(calls), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls)
    return lines


def test_obj_check_refusals_and_sizes(exe):
    got = run(exe, 'check', 'obj=0', 'conn=5', 'conn=0', 'area=0', 'area=-3', 'max=0', 'max=65536', 'n=0', 'table=0', 'table=4',
              'nx=1023,ny=1023,blocks=63,nthr=4', 'nx=1023,ny=1023,blocks=63,nthr=2')
    assert got[0] == 'off'
    assert got[1] == got[2] == 'refused connectivity must be 4 or 8'
    assert got[3] == got[4] == 'refused min_area must be at least 1'
    assert got[5] == got[6] == 'refused max_objects must lie in 1 ... 65535'
    assert got[7] == got[8] == 'refused n_objects or table is NULL'
    assert got[9] == 'refused table must be 8-byte aligned'
    # 64 sources x 4 thresholds of 1023 x 1023: the summed-area tables pass (1 GiB exactly), the labelling scratch does not; two
    # thresholds do, just
    assert got[10] == 'refused the labelling scratch of all blocks and thresholds must be at most 1 GiB'
    scratch = 64 * 2 * (2 * 1023 * 1023 + 1023) * 4
    assert scratch <= 1 << 30 and got[11].startswith('ok maps 128 cells %d scratch %d ' % (1023 * 1023, scratch))
    # the sizes and the grids of the measured case: 21 members and the observation, 300 x 300, three thresholds
    line, = run(exe, 'check', 'nx=300,ny=300,blocks=21,nthr=3,conn=8,area=4,max=1024,labels=1')
    maps, cells = 22 * 3, 90000
    assert line == 'ok maps %d cells %d scratch %d rows %d cellgroups %d decode %d n %d table %d labels %d' % (
        maps, cells, maps * (2 * cells + 300) * 4, 22 * 75, -(-maps * cells // 256), -(-maps * 1024 // 256), maps * 4,
        maps * 1024 * 40, maps * cells * 4)
    spec = spec_of(300, 300, [1, 2, 3])
    assert OB.scratch_bytes(spec, 21) == maps * (2 * cells + 300) * 4
    assert run(exe, 'check', 'nx=300,ny=300,blocks=21,nthr=3,labels=0')[0].endswith(' labels 0')
    assert run(exe, 'check', 'nx=7,ny=5,max=65535,nthr=4')[0] == 'ok maps 8 cells 35 scratch %d rows 4 cellgroups 2 decode 2048 n 32 table %d labels 0' % (
        8 * 75 * 4, 8 * 65535 * 40)


def test_host_build_of_runs_union_find_against_the_rule(exe, tmp_path):
    """The run, union and find code of cpol_obj.h, single-threaded, over the grids and patterns of the GPU tests."""
    rng = np.random.default_rng(14)
    files, want = [], []

    def case(binary, connectivity, min_area=1):
        n, _, lab = OB.cells_of_map(binary, np.zeros(binary.shape, f4), connectivity, min_area, 1)
        path = str(tmp_path / ('case%d.bin' % len(files)))
        with open(path, 'wb') as fh:
            np.array(binary.shape + (connectivity, min_area), i4).tofile(fh)
            binary.astype(u1).tofile(fh)
            lab.astype(i4).tofile(fh)
        files.append(path)
        want.append((int(n), len(OB._runs(binary)[0]), OB.label(binary, connectivity)[1]))
    for shape in SHAPES + [(257, 259)]:
        for connectivity, density in ((4, 0.59), (8, 0.41)):
            for min_area in (1, 2, 5):
                case(rng.random(shape) < density, connectivity, min_area)
            for name in PATTERNS:
                case(pattern(name, shape), connectivity)
    case(np.zeros((1, 1), bool), 4)
    case(np.ones((1, 1), bool), 8)
    lines = run(exe, 'label', *files)
    for line, (n, runs, roots) in zip(lines, want):
        assert line == 'ok objects %d runs %d roots %d' % (n, runs, roots)
    assert sum(r > o for _, r, o in want) > 50          # (merges happened: more runs than objects)
