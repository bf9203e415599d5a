"""Gridded composites without a GPU: the rule (cosmo_pol_amd/composite.py: `compose`, `finish`) against a plain Python loop over
the gates, its edge semantics one by one, the pass cut into calls, the helpers, every ValueError, the ctypes mirror of
cpol_composite against the header, and the host validation header (cosmo_pol_amd/csrc/cpol_comp.h) through
tests/c_host/comp_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program of its own.  All
comparisons are exact, NaNs positionally equal."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import composite as CP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
nan, inf = np.nan, np.inf


# ---------------------------------------------------------------------------------------------------- the plain loop
def key(f):
    b = struct.unpack('<I', struct.pack('<f', f))[0]
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def unkey(k):
    b = k ^ (0x80000000 if k >> 31 else 0xFFFFFFFF)
    return struct.unpack('<f', struct.pack('<I', b))[0]


def loop(spec, fields, dist, heights, az, rpb=0, states=None):
    """The rule, gate by gate, in Python integers and floats; (states, result)."""
    n_rays, ng = dist.shape
    ex, ey = [float(e) for e in spec.x_edges], [float(e) for e in spec.y_edges]
    nx, ny = len(ex) - 1, len(ey) - 1
    rows = next(iter(fields.values())).reshape(-1, ng).shape[0]
    nb = rows // rpb if rpb else 1
    per = rows // nb
    if states is None:
        states = {k: {'max': [0] * (nb * ny * nx), 'low': [2 ** 64 - 1] * (nb * ny * nx), 'count': [0] * (nb * ny * nx),
                      'top': [[0] * (nb * ny * nx) for _ in spec.thresholds[k]]} for k in spec.fields}
    for k in spec.fields:
        v = fields[k].reshape(-1, ng)
        st = states[k]
        for r in range(rows):
            ray = r % n_rays
            s, c = math.sin(math.radians(float(az[ray]))), math.cos(math.radians(float(az[ray])))
            assert s == np.sin(np.deg2rad(az[ray])) and c == np.cos(np.deg2rad(az[ray]))
            for g in range(ng):
                val, d, h = float(v[r, g]), float(dist[ray, g]), float(heights[ray, g])
                if val != val or d != d or h != h:
                    continue
                x, y = d * s, d * c
                ix = sum(1 for e in ex if e <= x) - 1
                iy = sum(1 for e in ey if e <= y) - 1
                if not (0 <= ix < nx and 0 <= iy < ny):
                    continue
                if spec.height_range is not None and not (float(spec.height_range[0]) <= h < float(spec.height_range[1])):
                    continue
                cell = (r // per) * ny * nx + iy * nx + ix
                kv, kh = key(val), key(h)
                st['count'][cell] += 1
                st['max'][cell] = max(st['max'][cell], kv << 32 | kh)
                st['low'][cell] = min(st['low'][cell], kh << 32 | kv)
                for j, t in enumerate(spec.thresholds[k]):
                    if val >= float(t):
                        st['top'][j][cell] = max(st['top'][j][cell], kh)
    out = {'values': {}, 'count': {}}
    sh = (nb, ny, nx)
    for k in spec.fields:
        st, planes = states[k], {}
        if 'max' in spec.products:
            planes['max'] = [unkey(s >> 32) if s else nan for s in st['max']]
            planes['height_of_max'] = [unkey(s & 0xFFFFFFFF) if s else nan for s in st['max']]
        if 'lowest' in spec.products:
            planes['lowest'] = [unkey(s & 0xFFFFFFFF) if s != 2 ** 64 - 1 else nan for s in st['low']]
            planes['height_of_lowest'] = [unkey(s >> 32) if s != 2 ** 64 - 1 else nan for s in st['low']]
        for j in range(len(spec.thresholds[k])):
            planes['echo_top_%d' % j] = [unkey(s) if s else nan for s in st['top'][j]]
        out['values'][k] = {p: np.array(a, dtype=F32).reshape(sh) for p, a in planes.items()}
        out['count'][k] = np.array(st['count'], dtype=np.uint64).reshape(sh)
    return states, out


def same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != F32:
        return np.array_equal(a, b)
    an, bn = np.isnan(a), np.isnan(b)
    return np.array_equal(an, bn) and np.array_equal(a[~an].view(np.uint32), b[~bn].view(np.uint32))


def assert_same(got, want, spec, tag=''):
    for k in spec.fields:
        assert list(got['values'][k]) == spec.planes(k) == list(want['values'][k]), (tag, k)
        for p in spec.planes(k):
            assert same(got['values'][k][p], want['values'][k][p]), (tag, k, p, got['values'][k][p], want['values'][k][p])
        assert same(got['count'][k], want['count'][k]), (tag, k, 'count')


SPECIAL = np.array([nan, inf, -inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, 3.0, 3.0, -3.0], dtype=F32)


def sweep(seed, n_rays, n_gates, ex, ey, rows=None):
    """A small sweep with ties in value and height, +-0.0, +-inf, denormals, NaN in the field, dist and height, gates on the
    edges of the grid (ray 0 points east: x = dist) and outside it."""
    rng = np.random.default_rng(seed)
    az = rng.uniform(0.0, 360.0, n_rays)
    az[0] = 90.0
    reach = max(abs(ex[0]), abs(ex[-1]), abs(ey[0]), abs(ey[-1]))
    dist = rng.uniform(0.0, 1.3 * reach, (n_rays, n_gates)).astype(F32)
    on = rng.random(n_gates) < 0.4
    dist[0, on] = rng.choice(np.asarray(ex, dtype=F32), int(on.sum()))
    dist[rng.random(dist.shape) < 0.05] = nan
    heights = rng.choice(np.array([-0.0, 0.0, 1e-45, 250.0, 1000.0, 1000.0, 2500.0, 4000.0, nan, inf], dtype=F32), (n_rays, n_gates))
    rows = rows or n_rays
    fields = {}
    for k in ('ZH', 'KDP'):
        v = rng.choice(np.arange(-4, 5).astype(F32) * F32(0.75), (rows, n_gates)).astype(F32)
        where = rng.random(v.shape) < 0.35
        v[where] = rng.choice(SPECIAL, int(where.sum()))
        fields[k] = v
    return fields, dist, heights, az


EX, EY = [0.0, 10.0, 25.0, 40.0], [-30.0, 0.0, 30.0]


def full_spec(**kw):
    return CP.Composite(['ZH', 'KDP'], EX, EY, products=('max', 'lowest', 'echo_top'),
                        thresholds={'ZH': [-1.0, 0.0, 0.75, 3.0], 'KDP': [0.0]}, **kw)


# ---------------------------------------------------------------------------------------------------- against the loop
@pytest.mark.parametrize('hr', [None, (250.0, 2500.0), (0.0, 1000.0), (-inf, inf)])
def test_rule_against_a_plain_loop(hr):
    spec = full_spec(height_range=hr)
    f, dist, heights, az = sweep(21, 5, 65, EX, EY)
    got = CP.finish(CP.compose(spec, f, dist, heights, az))
    _, want = loop(spec, f, dist, heights, az)
    assert_same(got, want, spec, hr)
    n = got['count']['ZH']
    assert n.shape == (1, 2, 3) and int((n > 0).sum()) >= 3
    # the case holds what it says: NaN in field, dist and height, both zeros, infinities, denormals, gates on every edge of x
    assert np.isnan(f['ZH']).any() and np.isnan(dist).any() and np.isnan(heights).any()
    assert all((dist[0] == F32(e)).any() for e in EX) and (dist > 45.0).any()
    assert np.isinf(f['ZH']).any() and (np.abs(f['ZH'][f['ZH'] != 0]) < 1e-38).any() and np.signbit(f['ZH'][f['ZH'] == 0]).any()


def test_blocks_and_the_geometry_of_an_ensemble_call():
    spec = full_spec()
    f, dist, heights, az = sweep(22, 3, 40, EX, EY, rows=6)        # two members over one geometry
    for rpb in (0, 3, 1):
        got = CP.finish(CP.compose(spec, f, dist, heights, az, rays_per_block=rpb))
        _, want = loop(spec, f, dist, heights, az, rpb)
        assert_same(got, want, spec, rpb)
        assert got['count']['ZH'].shape[0] == (6 // rpb if rpb else 1)
    per = CP.finish(CP.compose(spec, f, dist, heights, az, rays_per_block=3))
    whole = CP.finish(CP.compose(spec, f, dist, heights, az))
    assert np.array_equal(per['count']['ZH'].sum(axis=0, keepdims=True), whole['count']['ZH'])
    assert same(np.fmax.reduce(per['values']['ZH']['max'], axis=0, keepdims=True), whole['values']['ZH']['max'])
    # a member alone is its block
    one = CP.finish(CP.compose(spec, {k: v[3:] for k, v in f.items()}, dist, heights, az))
    assert all(same(one['values']['ZH'][p], per['values']['ZH'][p][1:]) for p in spec.planes('ZH'))
    shaped = CP.finish(CP.compose(spec, {k: v.reshape(2, 3, -1) for k, v in f.items()}, dist, heights, az, rays_per_block=3))
    assert_same(shaped, per, spec)
    with pytest.raises(ValueError):
        CP.compose(spec, f, dist, heights, az, rays_per_block=4)
    with pytest.raises(ValueError):
        CP.compose(spec, f, dist, heights, az, rays_per_block=-1)


def test_edge_semantics_by_hand():
    """One ray pointing east (sine exactly 1): x = dist.  Gates on the first, an inner and the last edge; ties; signed zeros."""
    ex, ey = [0.0, 1.0, 2.0, 3.0, 4.0], [-1.0, 1.0]
    dist = np.array([[0.0, 2.0, 4.0, 4.5, -0.0, 0.5, 0.5, 0.5, 1.5, 1.5, 1.5, 1.5, 2.5, 2.5, nan, 2.5, 2.5]], dtype=F32)
    hgt = np.array([[500., 500., 500., 500., 700., 100., 100., 900., 0.0, -0.0, 1e-45, 50., nan, 999., 500., 1000., 2000.]], dtype=F32)
    zh = np.array([[1.0, 1.0, 1.0, 1.0, nan, 2.0, 2.0, 2.0, -0.0, 0.0, -inf, inf, 5.0, 1e-45, 5.0, -1e-45, 7.0]], dtype=F32)
    spec = CP.Composite('ZH', ex, ey, products=('max', 'lowest', 'echo_top'), thresholds=[2.0, inf])
    got = CP.finish(CP.compose(spec, {'ZH': zh}, dist, hgt, [90.0]))
    assert_same(got, loop(spec, {'ZH': zh}, dist, hgt, [90.0])[1], spec)
    v, n = got['values']['ZH'], got['count']['ZH'][0, 0]
    assert n.tolist() == [4, 4, 4, 0]                    # the last edge is outside; the last cell stays empty
    assert all(np.isnan(v[p][0, 0, 3]) for p in spec.planes('ZH'))
    assert (v['max'][0, 0, 0], v['height_of_max'][0, 0, 0]) == (2.0, 900.0)            # ties in the value: the greater height
    assert (v['lowest'][0, 0, 0], v['height_of_lowest'][0, 0, 0]) == (2.0, 100.0)       # ties in the height: the smaller value ...
    assert np.signbit(v['height_of_lowest'][0, 0, 1]) and v['lowest'][0, 0, 1] == 0.0 and not np.signbit(v['lowest'][0, 0, 1])
    assert v['max'][0, 0, 1] == inf and v['height_of_max'][0, 0, 1] == 50.0
    assert (v['max'][0, 0, 2], v['height_of_max'][0, 0, 2], v['lowest'][0, 0, 2]) == (7.0, 2000.0, 1.0)
    assert v['echo_top_0'][0, 0].tolist()[:3] == [900.0, 50.0, 2000.0] and np.isnan(v['echo_top_1'][0, 0, 0]) and v['echo_top_1'][0, 0, 1] == 50.0
    # ... the smaller value, seen on its own: two gates at one height
    spec2 = CP.Composite('ZH', [0.0, 1.0], [-1.0, 1.0], products=('lowest',))
    g = CP.finish(CP.compose(spec2, {'ZH': np.array([[3.0, -2.0, 9.0]], dtype=F32)}, np.full((1, 3), 0.5, dtype=F32),
                             np.array([[10.0, 10.0, 20.0]], dtype=F32), [90.0]))
    assert g['values']['ZH']['lowest'].item() == -2.0 and g['values']['ZH']['height_of_lowest'].item() == 10.0
    # slab bounds hit exactly: [h_lo, h_hi)
    slab = CP.Composite('ZH', [0.0, 1.0], [-1.0, 1.0], height_range=(10.0, 20.0))
    h = np.array([[np.nextafter(F32(10), F32(0)), 10.0, np.nextafter(F32(20), F32(0)), 20.0]], dtype=F32)
    g = CP.finish(CP.compose(slab, {'ZH': np.array([[8.0, 1.0, 2.0, 9.0]], dtype=F32)}, np.full((1, 4), 0.5, dtype=F32), h, [90.0]))
    assert g['count']['ZH'].item() == 2 and g['values']['ZH']['max'].item() == 2.0
    # the bounds are the ROUNDED ones: 0.1 as float64 lies below float32(0.1), which the height float32(0.1) still reaches
    slab = CP.Composite('ZH', [0.0, 1.0], [-1.0, 1.0], height_range=(0.1, 1.0))
    g = CP.finish(CP.compose(slab, {'ZH': np.ones((1, 1), dtype=F32)}, np.full((1, 1), 0.5, dtype=F32), np.full((1, 1), 0.1, dtype=F32), [90.0]))
    assert g['count']['ZH'].item() == 1


def test_the_key_is_a_total_order_and_its_inverse_exact():
    v = np.array([-inf, -3.0, -1e-38, -1e-45, -0.0, 0.0, 1e-45, 1e-38, 3.0, inf], dtype=F32)
    k = CP.key32(v)
    assert k.dtype == np.uint32 and np.all(np.diff(k.astype(np.int64)) > 0)
    assert CP.unkey32(k).tobytes() == v.tobytes()
    assert [int(x) for x in k] == [key(float(x)) for x in v]
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32)
    f = bits.view(F32)
    f = f[f == f]
    assert CP.unkey32(CP.key32(f)).tobytes() == f.tobytes()
    assert np.array_equal(np.argsort(CP.key32(f), kind='stable'), np.lexsort((np.arange(f.size), np.signbit(f) == 0, f)))
    assert 0 not in CP.key32(f) and 0xFFFFFFFF not in CP.key32(f)
    assert np.isnan(CP.unkey32(np.array([0, 0xFFFFFFFF], dtype=np.uint32))).all()


# ---------------------------------------------------------------------------------------------------- the pass
@pytest.mark.parametrize('cut', [(1, 4), (2, 3), (1, 1, 1, 1, 1)])
def test_a_pass_cut_into_calls(cut):
    """A list of five sweeps of different shapes: however it is cut into calls, the bits are those of one call on the
    concatenation (sweeps of one gate count concatenated along the rays) and of the loop over all of them."""
    spec = full_spec(height_range=(0.0, 4000.0))
    sweeps = [sweep(30 + i, n_rays, 33, EX, EY) for i, n_rays in enumerate((3, 1, 4, 2, 5))]

    def join(part):
        return ({k: np.concatenate([s[0][k] for s in part]) for k in spec.fields}, np.concatenate([s[1] for s in part]),
                np.concatenate([s[2] for s in part]), np.concatenate([s[3] for s in part]))
    whole = CP.finish(CP.compose(spec, *join(sweeps)))
    state, at = None, 0
    for n in cut:
        state = CP.compose(spec, *join(sweeps[at:at + n]), state=state)
        at += n
    assert_same(CP.finish(state), whole, spec, cut)
    states = None
    for s in sweeps:
        states, want = loop(spec, *s, states=states)
    assert_same(whole, want, spec, 'loop')
    # calls of another gate count fold into the same pass when there is one block
    other = sweep(40, 2, 17, EX, EY)
    more = CP.finish(CP.compose(spec, *other, state=state))
    assert_same(more, loop(spec, *other, states=states)[1], spec, 'another gate count')
    with pytest.raises(ValueError):
        CP.compose(spec, *other, state=state, rays_per_block=1)
    with pytest.raises(ValueError):
        CP.compose(full_spec(), *other, state=state)


# ---------------------------------------------------------------------------------------------------- helpers
def test_helpers():
    e = CP.grid(150e3, 1e3)
    assert e.dtype == np.float64 and len(e) == 301 and e[0] == -150e3 and e[-1] == 150e3 and e[150] == 0.0
    assert np.array_equal(e, -150e3 + 1e3 * np.arange(301))
    assert len(CP.grid(10.0, 3.0)) == 8                 # round(20 / 3) = 7 cells
    for bad in ((0.0, 1.0), (1.0, 0.0), (1.0, -1.0), (1e6, 1.0), (inf, 1.0)):
        with pytest.raises(ValueError):
            CP.grid(*bad)
    assert np.array_equal(CP.from_db([0.0, 10.0, 35.0]), 10.0 ** (np.array([0.0, 10.0, 35.0]) / 10.0)) and CP.from_db(20.0) == 100.0
    assert np.array_equal(CP.centers([0.0, 1.0, 4.0]), [0.5, 2.5])
    spec = full_spec(height_range=(0.0, 1e4))
    assert spec.planes('ZH') == ['max', 'height_of_max', 'lowest', 'height_of_lowest', 'echo_top_0', 'echo_top_1', 'echo_top_2', 'echo_top_3']
    assert spec.planes('KDP')[-1] == 'echo_top_0' and len(spec.planes('KDP')) == 5
    assert CP.Composite('ZV', EX, EY).planes('ZV') == ['max', 'height_of_max']
    assert CP.Composite('ZV', EX, EY, products='lowest').planes('ZV') == ['lowest', 'height_of_lowest']
    assert CP.shape(spec, 'ZH', 6, 2) == (3, 8, 2, 3) and CP.shape(spec, 'KDP') == (1, 5, 2, 3) and CP.count_shape(spec, 6, 3) == (2, 2, 2, 3)
    assert (spec.mask, spec.product_mask, spec.n_x, spec.n_y) == (0b1001, 7, 3, 2)
    assert CP.Composite(['ATT_V'], EX, EY, products=('echo_top', 'max'), thresholds=[1.0]).product_mask == 5
    assert 'ZH' in repr(spec) and 'echo_top' in repr(spec) and 'height_range' in repr(spec)
    assert spec.key == full_spec(height_range=(0.0, 1e4)).key and spec == full_spec(height_range=(0.0, 1e4))
    assert spec != full_spec() and spec != full_spec(height_range=(0.0, 9e3)) and hash(spec) == hash(full_spec(height_range=(0.0, 1e4)))
    assert spec.thresholds['ZH'].dtype == F32 and spec.height_range[1].dtype == F32
    assert CP.FIELDS == ('ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V')
    assert (CP.MAX_EDGES, CP.MAX_THRESHOLDS, CP.MAX_STATE_BYTES) == (1024, 4, 1 << 30) and CP.STRETCH % 64 == 0
    # the state: per cell and block 8 bytes per count, 8 per max, 8 per lowest, 4 per threshold (padded to 8 per field)
    assert CP.state_bytes(spec, 1) == 2 * 6 * 24 + 6 * 16 + 6 * 4 and CP.state_bytes(spec, 5) == 2 * 30 * 24 + 30 * 16 + 30 * 4
    s, c = CP.ray_tables([0.0, 90.0, 180.0])
    assert s[1] == 1.0 and c[0] == 1.0 and s.dtype == np.float64 and c[2] == -1.0


@pytest.mark.parametrize('args', [
    dict(fields=[]), dict(fields=['ZX']), dict(fields=['RVEL']), dict(fields=['ZH', 'RVEL']),
    dict(x_edges=[1.0]), dict(x_edges=[[0.0, 1.0]]), dict(y_edges=[0.0, nan]), dict(y_edges=[0.0, inf]), dict(x_edges=[2.0, 1.0]),
    dict(x_edges=[1.0, 1.0]), dict(x_edges=np.arange(1025.0)), dict(y_edges=np.arange(1025.0)),
    dict(products=()), dict(products=('maximum',)), dict(products=('echo_top',)), dict(products=('max',), thresholds=[1.0]),
    dict(products=('echo_top',), thresholds=[]), dict(products=('echo_top',), thresholds=[1.0, 2.0, 3.0, 4.0, 5.0]),
    dict(products=('echo_top',), thresholds=[1.0, nan]), dict(products=('echo_top',), thresholds={'ZH': [1.0]}),
    dict(products=('echo_top',), thresholds={'ZH': [1.0], 'KDP': [1.0], 'ZV': [1.0]}),
    dict(height_range=(5.0, 5.0)), dict(height_range=(6.0, 5.0)), dict(height_range=(5.0, 5.0 + 1e-9)), dict(height_range=(nan, 5.0)),
    dict(height_range=(0.0, nan)),
])
def test_value_errors(args):
    kw = dict(fields=['ZH', 'KDP'], x_edges=EX, y_edges=EY)
    kw.update(args)
    with pytest.raises(ValueError):
        CP.Composite(**kw)


def test_limits():
    e = np.arange(1024.0)
    big = CP.Composite(list(CP.FIELDS), e, e, products=('max', 'lowest'))             # 1023 x 1023 cells, 9 fields: 226 MB a block
    assert CP.state_bytes(big, 1) == 1023 * 1023 * 9 * 24
    assert CP.state_bytes(big, 4) <= CP.MAX_STATE_BYTES < CP.state_bytes(big, 5)       # (the library refuses the fifth block)


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_struct_layout_matches_header(tmp_path):
    from cosmo_pol_amd import _native as N
    pairs = [('cpol_composite', N.Composite), ('cpol_histogram', N.Histogram), ('cpol_outputs', N.Outputs)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("fields %d thresholds %d bits %d %d %d\\n", CPOL_COMP_FIELDS, CPOL_COMP_MAX_THRESHOLDS, CPOL_COMP_MAX, '
                 'CPOL_COMP_LOWEST, CPOL_COMP_ECHO_TOP);')
    lines.append('cpol_outputs o; memset(&o, 0, sizeof o); printf("off %d\\n", o.composite == NULL);')
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    out = subprocess.check_output([exe]).decode().splitlines()
    got = dict(l.split() for l in out if len(l.split()) == 2)
    for cname, cls in pairs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert 'fields 9 thresholds 4 bits 1 2 4' in out and got['off'] == '1'
    assert len(N.COMPOSITE_FIELDS) == 9 and tuple(N.COMPOSITE_FIELDS) == CP.FIELDS and CP.PRODUCTS == ('max', 'lowest', 'echo_top')
    # composite sits directly before histogram, histogram directly before DSPECTRUM; the pinned tail is where it was
    names = [f for f, _ in N.Outputs._fields_]
    assert names[names.index('histogram') - 1] == 'composite' and names[names.index('DSPECTRUM') - 1] == 'histogram'
    assert names[-6:] == ['DSPECTRUM', 'member_verify', 'mask_sum8', 'spectrum_moments', 'member_stats', 'superob']
    assert names[:-2] == N.OUTPUT_FIELDS and names[names.index('composite') - 1] == 'sz_total'
    # a zero-initialised struct is "off", and the struct mirrors a spec
    assert not N.Outputs().composite
    spec = CP.Composite(['ZV', 'ATT_V'], EX, EY, products=('lowest', 'echo_top'), thresholds={'ZV': [1.0, 0.1], 'ATT_V': [5.0]},
                        height_range=(0.1, 2000.0))
    c, keep = N.Context.composite_struct(spec, phase=1, rays_per_block=4, azimuths=[0.0, 90.0])
    assert (c.fields, c.phase, c.products, c.rays_per_block, c.n_x, c.n_y, c.use_slab) == (0b100000010, 1, 6, 4, 3, 2, 1)
    assert list(c.n_thresholds) == [0, 2, 0, 0, 0, 0, 0, 0, 1] and list(c.thresholds[1])[:2] == [1.0, 0.1] and c.thresholds[8][0] == 5.0
    assert (c.h_lo, c.h_hi) == (0.1, 2000.0)             # as given: the library rounds
    assert c.edges_x and c.edges_y and c.ray_sin and c.ray_cos and not any(c.values) and not c.count
    c2, _ = N.Context.composite_struct(CP.Composite('ZH', EX, EY))
    assert (c2.fields, c2.products, c2.use_slab, c2.phase) == (1, 1, 0, 3) and not c2.ray_sin and not c2.ray_cos


# ---------------------------------------------------------------------------------------------------- the host validation header
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('comp') / 'comp_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'comp_check.cpp'),
                        '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def run(exe, *calls):
    r = subprocess.run([exe] + list(calls), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls)
    return lines


def lst(e):
    return ':'.join(float(x).hex() if np.isfinite(x) else repr(float(x)) for x in e)


def parse(line):
    assert line.startswith('ok '), line
    parts = line.split(' | ')
    w = parts[0].split()
    out = {}
    for name, x in zip(w[1::2], w[2::2]):
        out[name] = float.fromhex(x) if name in ('hlo', 'hhi') else int(x)
    out['fields'] = {}
    for p in parts[1:]:
        q = p.split()
        if q[0] == 'field':
            d = dict(zip(q[2:14:2], (int(x) for x in q[3:14:2])))
            d['thr'] = [float.fromhex(x) for x in q[15:]]
            out['fields'][int(q[1])] = d
        else:
            out[q[0]] = [float.fromhex(x) for x in q[2:]]
    return out


def test_host_header_plan_and_rounding(exe):
    ex, ey = [0.1, 0.2, 1.0 / 3.0, 7.0], [-1.0, 1e7 / 3.0]
    line, = run(exe, 'rows=12,gates=50,fields=0x9,products=7,rpb=3,hlo=0.1,hhi=1500.7;x=%s;y=%s;t0=0.1:1e39;t3=5' % (lst(ex), lst(ey)))
    p = parse(line)
    assert (p['blocks'], p['rpb'], p['cells'], p['begin'], p['finish'], p['open'], p['slab']) == (4, 3, 3, 1, 1, 0, 1)
    assert p['x'] == ex and p['y'] == ey                                        # float64: as given
    spec = CP.Composite(['ZH', 'KDP'], ex, ey, products=('max', 'lowest', 'echo_top'), thresholds={'ZH': [0.1, 1e39], 'KDP': [5.0]},
                        height_range=(0.1, 1500.7))
    assert (p['hlo'], p['hhi']) == tuple(float(x) for x in spec.height_range)     # rounded to float32, like NumPy
    assert p['fields'][0]['thr'] == [float(x) for x in spec.thresholds['ZH']] == [float(F32(0.1)), inf]
    assert p['fields'][3]['thr'] == [5.0]
    assert (p['fields'][0]['slot'], p['fields'][3]['slot'], p['fields'][0]['planes'], p['fields'][3]['planes']) == (0, 1, 6, 5)
    # the state: 12 (block, cell) pairs; per field max, count, tops (padded to 8 bytes), then every field's lowest
    per = 12
    f0, f3 = p['fields'][0], p['fields'][3]
    assert (f0['max'], f0['count'], f0['top']) == (0, per * 8, per * 16)
    assert (f3['max'], f3['count'], f3['top']) == (per * 24, per * 32, per * 40)
    assert p['zero'] == per * 44 and (f0['low'], f3['low']) == (per * 44, per * 52) and p['state'] == per * 60 == CP.state_bytes(spec, 4)
    # MAX alone: no tops, no lowest; an odd number of uint32 echo-top states is padded
    p = parse(run(exe, 'rows=7,gates=3,fields=0x4;x=1:2;y=0:1:2')[0])
    assert (p['blocks'], p['rpb'], p['cells'], p['state'], p['zero'], p['slab']) == (1, 7, 2, 32, 32, 0)
    assert (p['fields'][2]['max'], p['fields'][2]['count'], p['fields'][2]['top'], p['fields'][2]['low'], p['fields'][2]['planes']) == (0, 16, -1, -1, 2)
    p = parse(run(exe, 'fields=0x1,products=4;x=1:2;y=0:1;t0=1:2:3')[0])
    assert (p['fields'][0]['max'], p['fields'][0]['count'], p['fields'][0]['top'], p['state'], p['fields'][0]['planes']) == (-1, 0, 8, 24, 3)
    p = parse(run(exe, 'fields=0x3,products=2;x=1:2;y=0:1')[0])
    assert (p['zero'], p['state'], p['fields'][0]['low'], p['fields'][1]['low']) == (16, 32, 16, 24)


def test_host_header_limits(exe):
    e1024 = lst(np.arange(1024.0))
    assert parse(run(exe, 'fields=0x1;x=%s;y=%s' % (e1024, e1024))[0])['cells'] == 1023 * 1023
    assert '1024' in run(exe, 'fields=0x1;x=%s;y=0:1' % lst(np.arange(1025.0)))[0]
    assert '1024' in run(exe, 'fields=0x1;x=0:1;y=%s' % lst(np.arange(1025.0)))[0]
    assert '1024' in run(exe, 'fields=0x1,nx=1024;x=0:1;y=0:1')[0]
    # 1 GiB of state: 1023 x 1023 cells, 9 fields, max + lowest (24 bytes): 4 blocks fit, 5 do not
    big = 'rows=%d,rpb=1,fields=0x1ff,products=3;x=%s;y=%s'
    assert parse(run(exe, big % (4, e1024, e1024))[0])['state'] == 4 * 1023 * 1023 * 9 * 24
    assert '1 GiB' in run(exe, big % (5, e1024, e1024))[0]
    # 2^31 workgroups: out of reach of a call below 2^31 gates, so the arithmetic alone: one block of 2^31 stretches
    assert 'too many workgroups' in run(exe, 'rows=2147483648,gates=1024,fields=0x1;x=0:1;y=0:1')[0]
    assert run(exe, 'rows=2147483647,gates=1024,fields=0x1;x=0:1;y=0:1')[0].startswith('ok ')


def test_host_header_refusals(exe):
    ok = 'fields=0x1;x=1:2;y=0:1'
    cases = {
        'phase=4,' + ok: 'phase', 'phase=-1,' + ok: 'phase',
        'fields=0;x=1:2;y=0:1': 'fields', 'fields=0x400;x=1:2;y=0:1': 'fields', 'fields=0x200;x=1:2;y=0:1': 'RVEL',
        'fields=0x201;x=1:2;y=0:1': 'RVEL',
        'products=0,' + ok: 'products', 'products=8,' + ok: 'products', 'products=9,' + ok: 'products',
        'products=4,' + ok: '1 ... 4 thresholds', 'products=4,n0=5,' + ok: '1 ... 4 thresholds', 'products=4,' + ok + ';t0=1:2:3:4:5': '1 ... 4 thresholds',
        'products=4,fields=0x3;x=1:2;y=0:1;t0=1': '1 ... 4 thresholds',
        'products=1,' + ok + ';t0=1': 'thresholds without', 'products=4,' + ok + ';t0=1:nan': 'NaN',
        'hlo=5,hhi=5,' + ok: 'h_lo < h_hi', 'hlo=6,hhi=5,' + ok: 'h_lo < h_hi', 'hlo=5,hhi=5.0000000001,' + ok: 'h_lo < h_hi',
        'hlo=nan,' + ok: 'h_lo < h_hi', 'hhi=nan,' + ok: 'h_lo < h_hi', 'hlo=inf,' + ok: 'h_lo < h_hi', 'hlo=1e39,hhi=2e39,' + ok: 'h_lo < h_hi',
        'fields=0x1,nx=0;x=1:2;y=0:1': 'n_x and n_y', 'fields=0x1,ny=0;x=1:2;y=0:1': 'n_x and n_y', 'fields=0x1;x=1:2': 'n_x and n_y',
        'fields=0x1;x=null;y=0:1': 'NULL', 'fields=0x1;x=1:2;y=null': 'NULL',
        'fields=0x1;x=1:nan;y=0:1': 'NaN or infinite', 'fields=0x1;x=1:2;y=0:inf': 'NaN or infinite', 'fields=0x1;x=-inf:1;y=0:1': 'NaN or infinite',
        'fields=0x1;x=2:1;y=0:1': 'ascending', 'fields=0x1;x=1:1;y=0:1': 'ascending', 'fields=0x1;x=1:2;y=0:1:1': 'ascending',
        'rays=0,' + ok: 'ray_sin', 'rows=6,rpb=-1,' + ok: 'rays_per_block', 'rows=6,rpb=4,' + ok: 'rays_per_block',
        'phase=0,' + ok: 'no pass open', 'phase=2,' + ok: 'no pass open',
        'count=0,' + ok: 'count', 'values=0,' + ok: 'values', 'space=1,' + ok: 'spaceborne',
    }
    for call, word in cases.items():
        line, = run(exe, call)
        assert line.startswith('refused ') and word in line, (call, line)
    # float64 edges keep what float32 would collapse; infinite slab bounds and thresholds are taken; no outputs before the finish
    assert run(exe, 'fields=0x1;x=1:1.000000001:2;y=0:1')[0].startswith('ok ')
    assert parse(run(exe, 'hlo=-inf,hhi=inf,' + ok)[0])['slab'] == 1 and parse(run(exe, 'hhi=1e39,' + ok)[0])['hhi'] == inf
    assert parse(run(exe, 'products=4,' + ok + ';t0=-inf:inf:1e39')[0])['fields'][0]['thr'] == [-inf, inf, inf]
    assert run(exe, 'count=0,values=0,phase=1,' + ok)[0].startswith('ok ')


def test_host_header_pass(exe):
    a = 'rows=4,fields=0x3,products=7,hlo=0,hhi=9000,phase=%d;x=1:2:3;y=0:10;t0=1:2;t1=3'
    out = run(exe, a % 1, a % 0, 'gates=9,rows=11,fields=0x3,products=7,hlo=0,hhi=9000,phase=0;x=1:2:3;y=0:10;t0=1:2;t1=3', a % 2, a % 0)
    assert [parse(l)['open'] for l in out[:4]] == [1, 1, 1, 0] and out[4].startswith('refused') and 'no pass open' in out[4]
    # what differs from the open pass is refused and leaves it open: the call after it still finishes
    for other in ('rows=4,fields=0x1,products=7,hlo=0,hhi=9000,phase=0;x=1:2:3;y=0:10;t0=1:2',                 # fields
                  'rows=4,fields=0x3,products=3,hlo=0,hhi=9000,phase=0;x=1:2:3;y=0:10',                        # products
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9001,phase=0;x=1:2:3;y=0:10;t0=1:2;t1=3',             # the slab
                  'rows=4,fields=0x3,products=7,phase=0;x=1:2:3;y=0:10;t0=1:2;t1=3',                           # no slab
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9000.0000001,phase=0;x=1:2:3;y=0:10;t0=1:2;t1=3',     # rounds to the same float32: accepted
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9000,phase=0;x=1:2:3;y=0:10;t0=1:2.5;t1=3',           # a threshold
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9000,phase=0;x=1:2:3;y=0:10;t0=1:2:3;t1=3',           # one threshold more
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9000,phase=0;x=1:2:3;y=0:10;t0=1:2.0000000001;t1=3',   # the same float32: accepted
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9000,phase=0;x=1:2:4;y=0:10;t0=1:2;t1=3',             # an edge
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9000,phase=0;x=1:2:3.0000001;y=0:10;t0=1:2;t1=3',     # float64 edges: another edge
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9000,phase=0;x=1:2:3;y=0:11;t0=1:2;t1=3',             # a y edge
                  'rows=4,rpb=2,fields=0x3,products=7,hlo=0,hhi=9000,phase=0;x=1:2:3;y=0:10;t0=1:2;t1=3',       # blocks
                  'rows=4,fields=0x3,products=7,hlo=0,hhi=9000,phase=7;x=1:2:3;y=0:10;t0=1:2;t1=3'):            # any refusal
        out = run(exe, a % 1, other, a % 2)
        accepted = '9000.0000001' in other or '2.0000000001' in other
        assert out[1].startswith('ok ' if accepted else 'refused '), (other, out[1])
        if not accepted and 'phase=7' not in other:
            assert 'differ' in out[1], (other, out[1])
        assert parse(out[2])['open'] == 0 and parse(out[0])['open'] == 1
    # with blocks every call gives the same number of them, whatever its rows
    b = 'rows=%d,rpb=%d,fields=0x1,phase=%d;x=1:2;y=0:1'
    out = run(exe, b % (6, 2, 1), b % (9, 3, 0), b % (8, 2, 0), b % (6, 2, 2))
    assert out[0].startswith('ok') and out[1].startswith('ok') and 'differ' in out[2] and parse(out[3])['open'] == 0
    # a begin in the middle starts over
    out = run(exe, a % 1, 'fields=0x4,phase=1;x=1:2;y=0:1', 'fields=0x4,phase=2;x=1:2;y=0:1')
    assert all(l.startswith('ok') for l in out)
