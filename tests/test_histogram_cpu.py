"""Sweep histograms without a GPU: the rule (cosmo_pol_amd/histogram.py: `count`) against np.histogram / np.histogram2d where
the two conventions agree and against hand-counted cells where they do not, its edge semantics one by one, the pass, the
helpers, every ValueError, the ctypes mirror of cpol_histogram against the header, and the host validation header
(cosmo_pol_amd/csrc/cpol_hist.h) through tests/c_host/hist_check.cpp, built with the address and undefined-behaviour
sanitizers and run as a program of its own.  All comparisons are exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import histogram as HG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def nxt(x, to):
    return np.nextafter(F32(x), F32(to))


# ---------------------------------------------------------------------------------------------------- against NumPy
def test_count_1d_against_np_histogram():
    rng = np.random.default_rng(11)
    edges = np.array([-2.0, -0.5, 0.0, 0.25, 1.0, 3.0])
    v = rng.normal(0.0, 1.5, (7, 93)).astype(F32)
    e32 = edges.astype(F32)
    v[v == e32[-1]] = 0.1                              # (no value on the last edge: np.histogram closes its last bin)
    spec = HG.Histogram({'ZH': edges})
    c = HG.count({'ZH': v}, spec)['ZH']
    assert c.shape == (1, 7) and c.dtype == np.uint64
    want, _ = np.histogram(v, bins=e32)
    assert np.array_equal(c[0, 1:-1], want.astype(np.uint64))
    assert c[0, 0] == np.sum(v < e32[0]) and c[0, -1] == np.sum(v >= e32[-1])
    assert c.sum() == v.size


def test_count_2d_against_np_histogram2d():
    rng = np.random.default_rng(12)
    ex = np.array([0.1, 0.5, 1.0, 2.0, 8.0])
    ey = np.array([0.0, 1000.0, 2500.0, 6000.0])
    v = rng.gamma(2.0, 1.0, (5, 64)).astype(F32)
    y = rng.uniform(-500.0, 7000.0, (5, 64)).astype(F32)
    v[rng.random(v.shape) < 0.1] = np.nan
    y[rng.random(y.shape) < 0.1] = np.nan
    spec = HG.Histogram({'KDP': ex}, ordinate='heights', ordinate_edges=ey)
    c = HG.count({'KDP': v, 'heights': y}, spec)['KDP']
    assert c.shape == (1, 5, 6)
    ok = (v == v) & (y == y)
    want, _, _ = np.histogram2d(y[ok], v[ok], bins=(ey.astype(F32), ex.astype(F32)))
    assert np.array_equal(c[0, 1:-1, 1:-1], want.astype(np.uint64))
    assert c.sum() == ok.sum()
    # under- and overflow from explicit masks
    e32, y32 = ex.astype(F32), ey.astype(F32)
    assert c[0, :, 0].sum() == np.sum(ok & (v < e32[0])) and c[0, :, -1].sum() == np.sum(ok & (v >= e32[-1]))
    assert c[0, 0, :].sum() == np.sum(ok & (y < y32[0])) and c[0, -1, :].sum() == np.sum(ok & (y >= y32[-1]))


def test_rvel_is_float64_and_field_as_ordinate():
    rng = np.random.default_rng(13)
    rv = rng.normal(0, 8, (4, 50))
    zh = rng.gamma(1.0, 50.0, (4, 50)).astype(F32)
    e = np.array([-10.0, 0.0, 0.1 + 1e-12, 10.0])       # (an edge float32 would move: RVEL keeps it)
    spec = HG.Histogram({'RVEL': e, 'ZH': [1.0, 10.0, 100.0]}, ordinate='RVEL', ordinate_edges=e)
    assert spec.edges['RVEL'].dtype == np.float64 and spec.edges['ZH'].dtype == F32 and spec.ordinate_edges.dtype == np.float64
    assert spec.edges['RVEL'][2] == 0.1 + 1e-12
    c = HG.count({'RVEL': rv, 'ZH': zh}, spec)
    assert c['RVEL'].shape == (1, 5, 5) and c['ZH'].shape == (1, 5, 4)
    ix = np.searchsorted(e, rv, side='right')
    for i in range(5):                                  # a field against itself: the diagonal alone
        assert c['RVEL'][0, i, i] == np.sum(ix == i)
    assert c['RVEL'].sum() == rv.size == np.trace(c['RVEL'][0])
    with pytest.raises(ValueError):
        HG.count({'RVEL': rv.astype(F32), 'ZH': zh}, spec)


# ---------------------------------------------------------------------------------------------------- edge semantics
def one(v, edges, field='ZH'):
    dt = HG.dtype_of(field)
    return HG.count({field: np.array([[v]], dtype=dt)}, HG.Histogram({field: edges}))[field][0]


def test_value_on_an_edge_and_its_float32_neighbours():
    edges = [1.0, 2.0, 4.0]
    assert one(2.0, edges).tolist() == [0, 0, 1, 0]                      # on an edge: the bin above
    assert one(nxt(2.0, 0), edges).tolist() == [0, 1, 0, 0]
    assert one(nxt(2.0, 9), edges).tolist() == [0, 0, 1, 0]
    assert one(1.0, edges).tolist() == [0, 1, 0, 0] and one(nxt(1.0, 0), edges).tolist() == [1, 0, 0, 0]
    assert one(4.0, edges).tolist() == [0, 0, 0, 1] and one(nxt(4.0, 0), edges).tolist() == [0, 0, 1, 0]   # the last edge: overflow
    # the edge is the ROUNDED one: 0.1 as float64 lies below float32(0.1); the float32 value 0.1 sits on the rounded edge
    assert one(F32(0.1), [0.1, 1.0]).tolist() == [0, 1, 0]
    assert one(nxt(0.1, 0), [0.1, 1.0]).tolist() == [1, 0, 0]


def test_signed_zeros_and_infinities():
    edges = [-1.0, 0.0, 1.0]
    assert one(-0.0, edges).tolist() == [0, 0, 1, 0] and one(0.0, edges).tolist() == [0, 0, 1, 0]
    assert one(-0.0, [-1.0, -0.0, 1.0]).tolist() == [0, 0, 1, 0]          # an edge at -0.0 is the same edge
    assert one(np.inf, edges).tolist() == [0, 0, 0, 1] and one(-np.inf, edges).tolist() == [1, 0, 0, 0]
    assert one(np.inf, edges, 'RVEL').tolist() == [0, 0, 0, 1] and one(-0.0, edges, 'RVEL').tolist() == [0, 0, 1, 0]


def test_nan_in_field_ordinate_and_both():
    nan = np.nan
    v = np.array([[1.5, nan, 1.5, nan, 0.5]], dtype=F32)
    y = np.array([[10.0, 10.0, nan, nan, -5.0]], dtype=F32)
    spec = HG.Histogram({'ZH': [1.0, 2.0]}, ordinate='dist', ordinate_edges=[0.0, 20.0])
    c = HG.count({'ZH': v, 'dist': y}, spec)['ZH'][0]
    want = np.zeros((3, 3), dtype=np.uint64)
    want[1, 1] = 1                                     # (1.5, 10)
    want[0, 0] = 1                                     # (0.5, -5): under both
    assert np.array_equal(c, want)
    assert one(nan, [1.0, 2.0]).sum() == 0
    # without the ordinate only the field's NaN matters
    assert HG.count({'ZH': v}, HG.Histogram({'ZH': [1.0, 2.0]}))['ZH'][0].tolist() == [1, 2, 0]


def test_edges_that_collapse_in_float32_are_refused():
    with pytest.raises(ValueError, match='ascending'):
        HG.Histogram({'ZH': [1.0, 1.0 + 1e-9, 2.0]})
    HG.Histogram({'RVEL': [1.0, 1.0 + 1e-9, 2.0]})      # float64 keeps them apart
    with pytest.raises(ValueError, match='ascending'):
        HG.Histogram({'RVEL': [1.0, 2.0]}, ordinate='ZH', ordinate_edges=[1.0, 1.0 + 1e-9])
    HG.Histogram({'ZH': [1.0, 2.0]}, ordinate=('model', 'T'), ordinate_edges=[1.0, 1.0 + 1e-9])


# ---------------------------------------------------------------------------------------------------- blocks and the pass
def rows(seed, n_rows, n_gates=40):
    rng = np.random.default_rng(seed)
    v = rng.gamma(1.5, 2.0, (n_rows, n_gates)).astype(F32)
    v[rng.random(v.shape) < 0.15] = np.nan
    h = rng.uniform(0, 9000, (n_rows, n_gates)).astype(F32)
    return {'ZH': v, 'ZV': (v * F32(0.7)).astype(F32), 'heights': h}


SPEC = HG.Histogram({'ZH': [0.5, 1.0, 2.0, 4.0], 'ZV': [1.0, 3.0]}, ordinate='heights', ordinate_edges=[0.0, 3000.0, 6000.0])


def test_blocks():
    pg = rows(1, 6)
    whole = HG.count(pg, SPEC)
    per_ray = HG.count(pg, SPEC, rays_per_block=1)
    pairs = HG.count(pg, SPEC, rays_per_block=2)
    assert per_ray['ZH'].shape == (6, 4, 5) and pairs['ZV'].shape == (3, 4, 3) and HG.shape(SPEC, 'ZH', 6, 2) == (3, 4, 5)
    for k in SPEC.fields:
        assert np.array_equal(per_ray[k].sum(axis=0, keepdims=True), whole[k])
        assert np.array_equal(per_ray[k].reshape(3, 2, *per_ray[k].shape[1:]).sum(axis=1), pairs[k])
        for r in range(6):
            assert np.array_equal(per_ray[k][r:r + 1], HG.count({q: a[r:r + 1] for q, a in pg.items()}, SPEC)[k])
    with pytest.raises(ValueError):
        HG.count(pg, SPEC, rays_per_block=4)
    with pytest.raises(ValueError):
        HG.count(pg, SPEC, rays_per_block=-1)


def test_ordinate_of_an_ensemble_call_is_taken_row_mod_n_rays():
    pg = rows(2, 6)
    geo = {'ZH': pg['ZH'], 'ZV': pg['ZV'], 'heights': pg['heights'][:2]}       # 3 members x 2 rays, the geometry once
    full = {'ZH': pg['ZH'], 'ZV': pg['ZV'], 'heights': np.tile(pg['heights'][:2], (3, 1))}
    a, b = HG.count(geo, SPEC, rays_per_block=2, n_rays=2), HG.count(full, SPEC, rays_per_block=2)
    assert all(np.array_equal(a[k], b[k]) for k in SPEC.fields)
    shaped = {'ZH': pg['ZH'].reshape(3, 2, -1), 'ZV': pg['ZV'].reshape(3, 2, -1), 'heights': pg['heights'][:2]}
    c = HG.count(shaped, SPEC, rays_per_block=2)
    assert all(np.array_equal(a[k], c[k]) for k in SPEC.fields)


def test_a_pass_cut_into_calls():
    pg = rows(3, 3)
    whole = HG.count(pg, SPEC)
    first = HG.count({k: a[:1] for k, a in pg.items()}, SPEC)
    second = HG.count({k: a[1:] for k, a in pg.items()}, SPEC)
    state = HG.count({k: a[:1] for k, a in pg.items()}, SPEC)
    back = HG.count({k: a[1:] for k, a in pg.items()}, SPEC, into=state)
    assert back is state
    for k in SPEC.fields:
        assert np.array_equal(first[k] + second[k], whole[k]) and np.array_equal(state[k], whole[k])
    # a call of another gate count folds into the same pass when there is one block
    other = rows(4, 2, n_gates=17)
    HG.count(other, SPEC, into=state)
    assert state['ZH'].sum() == whole['ZH'].sum() + HG.count(other, SPEC)['ZH'].sum()
    with pytest.raises(ValueError):
        HG.count(pg, SPEC, rays_per_block=1, into=state)


# ---------------------------------------------------------------------------------------------------- helpers
def test_db_edges_frequencies_centers_shape():
    e = HG.db_edges(-10, 50, 1)
    assert e.dtype == np.float64 and len(e) == 61
    assert np.array_equal(e, 10.0 ** ((-10.0 + np.arange(61)) / 10.0)) and e[10] == 1.0 and e[0] == 0.1
    assert len(HG.db_edges(0, 1, 0.3)) == 4             # 0, 0.3, 0.6, 0.9: never beyond hi
    with pytest.raises(ValueError):
        HG.db_edges(5, 5, 1)
    with pytest.raises(ValueError):
        HG.db_edges(0, 5, 0)
    c = np.array([[[1, 3, 0], [0, 0, 0], [2, 2, 4]]], dtype=np.uint64)
    f = HG.frequencies(c)
    assert np.array_equal(f[0, 0], [0.25, 0.75, 0.0]) and np.all(np.isnan(f[0, 1])) and np.array_equal(f[0, 2], [0.25, 0.25, 0.5])
    assert np.array_equal(HG.centers([0.0, 1.0, 4.0]), [0.5, 2.5])
    s1 = HG.Histogram({'ZDR': [1.0, 2.0, 3.0]})
    assert HG.shape(s1, 'ZDR') == (1, 4) and HG.shape(s1, 'ZDR', 8, 2) == (4, 4) and HG.shape(SPEC, 'ZV', 5, 1) == (5, 4, 3)
    assert SPEC.cells == 4 * 5 + 4 * 3 and SPEC.mask == 0b11 and s1.mask == 0b100
    assert 'ZH' in repr(SPEC) and 'heights' in repr(SPEC)
    assert SPEC.key == HG.Histogram({'ZV': [1.0, 3.0], 'ZH': [0.5, 1.0, 2.0, 4.0]}, 'heights', [0.0, 3000.0, 6000.0]).key
    assert SPEC.key != HG.Histogram({'ZV': [1.0, 3.0], 'ZH': [0.5, 1.0, 2.0, 4.0]}, 'dist', [0.0, 3000.0, 6000.0]).key
    assert HG.FIELDS == ('ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL')
    assert (HG.MAX_EDGES, HG.MAX_CELLS, HG.MAX_STATE_CELLS) == (1024, 16384, 1 << 27) and 0 < HG.STRETCH < 2 ** 32


@pytest.mark.parametrize('args', [
    dict(fields={}), dict(fields={'ZX': [1.0, 2.0]}), dict(fields={'ZH': [1.0]}), dict(fields={'ZH': [[1.0, 2.0]]}),
    dict(fields={'ZH': [1.0, np.nan]}), dict(fields={'ZH': [1.0, np.inf]}), dict(fields={'ZH': [1.0, 1e39]}),
    dict(fields={'ZH': [2.0, 1.0]}), dict(fields={'ZH': [1.0, 1.0]}), dict(fields={'ZH': np.arange(1025.0)}),
    dict(fields={'ZH': [1.0, 2.0]}, ordinate='height', ordinate_edges=[0.0, 1.0]),
    dict(fields={'ZH': [1.0, 2.0]}, ordinate='heights'), dict(fields={'ZH': [1.0, 2.0]}, ordinate_edges=[0.0, 1.0]),
    dict(fields={'ZH': [1.0, 2.0]}, ordinate=('model',), ordinate_edges=[0.0, 1.0]),
    dict(fields={'ZH': [1.0, 2.0]}, ordinate='heights', ordinate_edges=[0.0, -1.0]),
    dict(fields={'ZH': np.arange(127.0)}, ordinate='heights', ordinate_edges=np.arange(128.0)),       # 128 * 129 cells
])
def test_value_errors(args):
    with pytest.raises(ValueError):
        HG.Histogram(**args)


def test_the_largest_table_is_accepted():
    s = HG.Histogram({'ZH': np.arange(127.0)}, ordinate='heights', ordinate_edges=np.arange(127.0))
    assert s.cells == 16384
    assert len(HG.Histogram({'ZH': np.arange(1024.0)}).edges['ZH']) == 1024


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_struct_layout_matches_header(tmp_path):
    from cosmo_pol_amd import _native as N
    pairs = [('cpol_histogram', N.Histogram), ('cpol_outputs', N.Outputs)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cosmo_pol_amd.h"', 'int main(void){']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("fields %d\\n", CPOL_HIST_FIELDS);')
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert int(got['fields']) == len(N.HISTOGRAM_FIELDS) == len(HG.FIELDS) and tuple(N.HISTOGRAM_FIELDS) == HG.FIELDS
    # histogram sits directly before DSPECTRUM (every member from there on is pinned where it is); superob stays last
    names = [f for f, _ in N.Outputs._fields_]
    assert names[names.index('DSPECTRUM') - 1] == 'histogram' and names[-1] == 'superob'
    # a zero-initialised struct is "off", and the struct mirrors a spec
    spec = HG.Histogram({'ZV': [1.0, 2.0, 3.0], 'RVEL': [0.0, 1.0]}, ordinate=('model', 'T'), ordinate_edges=[250.0, 260.0, 273.15])
    h, keep = N.Context.histogram_struct(spec, phase=1, rays_per_block=4, model_index=5)
    assert (h.fields, h.phase, h.ordinate, h.n_y, h.rays_per_block) == (0b1000000010, 1, 32 + 5, 2, 4)
    assert list(h.n_x) == [0, 2, 0, 0, 0, 0, 0, 0, 0, 1] and h.edges_x[1] and h.edges_x[9] and not h.edges_x[0] and h.edges_y
    assert not any(h.counts)
    h2, _ = N.Context.histogram_struct(HG.Histogram({'ZH': [1.0, 2.0]}, 'KDP', [0.0, 1.0]))
    assert (h2.ordinate, HG.Histogram({'ZH': [1.0, 2.0]}, 'dist', [0.0, 1.0]).ordinate) == (16 + 3, 'dist')
    with pytest.raises(ValueError):
        N.Context.histogram_struct(spec)                 # a model ordinate without its index


# ---------------------------------------------------------------------------------------------------- the host validation header
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('hist') / 'hist_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'hist_check.cpp'),
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
    out = dict(zip(w[1::2], (int(x) for x in w[2::2])))
    out['fields'] = {}
    for p in parts[1:]:
        q = p.split()
        if q[0] == 'field':
            out['fields'][int(q[1])] = dict(cells=int(q[3]), off=int(q[5]), edges=[float.fromhex(x) for x in q[7:]])
        else:
            out['y'] = [float.fromhex(x) for x in q[2:]]
    return out


def test_host_header_plan_and_rounding(exe):
    ex0 = [0.1, 0.2, 1.0 / 3.0, 7.0]
    ex9 = [0.1, 0.2, 1.0 / 3.0]
    ey = [0.0, 1500.5, 1e7 / 3.0]
    line, = run(exe, 'rows=12,gates=50,fields=0x201,ord=1,rpb=3;x0=%s;x9=%s;y=%s' % (lst(ex0), lst(ex9), lst(ey)))
    p = parse(line)
    assert (p['blocks'], p['rpb'], p['begin'], p['finish'], p['open']) == (4, 3, 1, 1, 0)
    spec = HG.Histogram({'ZH': ex0, 'RVEL': ex9}, ordinate='heights', ordinate_edges=ey)
    assert p['fields'][0]['edges'] == [float(x) for x in spec.edges['ZH']]          # rounded to float32, like NumPy
    assert p['fields'][9]['edges'] == ex9                                          # float64: as given
    assert p['y'] == [float(x) for x in spec.ordinate_edges]
    assert p['fields'][0]['cells'] == 5 * 4 and p['fields'][9]['cells'] == 4 * 4
    assert p['fields'][0]['off'] == 0 and p['fields'][9]['off'] == 4 * 20 and p['state'] == 4 * 36 == 4 * spec.cells
    # no ordinate, one block
    p = parse(run(exe, 'rows=7,gates=3,fields=0x4;x2=1:2')[0])
    assert (p['blocks'], p['rpb'], p['state']) == (1, 7, 3) and p['fields'][2]['cells'] == 3
    # ordinate codes
    for ord_, extra in ((2, ''), (16, ''), (16 + 9, ''), (32, ',nmv=1'), (32 + 4, ',nmv=5')):
        assert run(exe, 'fields=0x1,ord=%d%s;x0=1:2;y=0:1' % (ord_, extra))[0].startswith('ok ')


def test_host_header_limits(exe):
    e1024, e127, e128 = lst(np.arange(1024.0)), lst(np.arange(127.0)), lst(np.arange(128.0))
    assert parse(run(exe, 'fields=0x1;x0=' + e1024)[0])['fields'][0]['cells'] == 1025
    assert run(exe, 'fields=0x1;x0=' + lst(np.arange(1025.0)))[0].startswith('refused n_x + 1')
    assert parse(run(exe, 'fields=0x1,ord=1;x0=%s;y=%s' % (e127, e127))[0])['fields'][0]['cells'] == 16384
    assert '16384 cells' in run(exe, 'fields=0x1,ord=1;x0=%s;y=%s' % (e127, e128))[0]
    assert '16384 cells' in run(exe, 'fields=0x1,ord=1;x0=%s;y=%s' % (e128, e127))[0]
    assert run(exe, 'fields=0x1,ord=1;x0=1:2;y=' + lst(np.arange(1025.0)))[0].startswith('refused n_y + 1')
    # 2^27 cells of state: 8192 blocks of 16384 cells fit, one field more does not
    big = 'rows=8192,rpb=1,ord=1,fields=%s;x0=%s;x1=1:2;y=%s'
    assert parse(run(exe, big % ('0x1', e127, e127))[0])['state'] == 1 << 27
    assert '2^27' in run(exe, big % ('0x3', e127, e127))[0]


def test_host_header_refusals(exe):
    ok = 'fields=0x1;x0=1:2'
    cases = {
        'phase=4,' + ok: 'phase', 'phase=-1,' + ok: 'phase',
        'fields=0;x0=1:2': 'fields', 'fields=0x400;x0=1:2': 'fields',
        'dop=0,fields=0x200;x9=1:2': 'RVEL', 'dop=0,fields=0x1,ord=25;x0=1:2;y=0:1': 'RVEL',
        'fields=0x1,ord=3;x0=1:2;y=0:1': 'unknown ordinate', 'fields=0x1,ord=26;x0=1:2;y=0:1': 'unknown ordinate',
        'fields=0x1,ord=56;x0=1:2;y=0:1': 'unknown ordinate', 'fields=0x1,ord=-1;x0=1:2;y=0:1': 'unknown ordinate',
        'fields=0x1,ord=32;x0=1:2;y=0:1': 'model', 'fields=0x1,ord=34,nmv=2;x0=1:2;y=0:1': 'beyond n_vars',
        'fields=0x1,ord=1,ny=0;x0=1:2;y=0:1': 'n_y >= 1', 'fields=0x1,ord=1,ny=1;x0=1:2': 'edges_y',
        'fields=0x1,ord=0,ny=1;x0=1:2': 'n_y must be 0',
        'fields=0x1,nx0=0;x0=1:2': 'n_x', 'fields=0x1,nx0=1024;x0=1:2': 'n_x + 1',
        'fields=0x1;x0=null': 'NULL', 'fields=0x3;x0=1:2': 'n_x',
        'fields=0x1;x0=1:nan': 'NaN or infinite', 'fields=0x1;x0=1:inf': 'NaN or infinite', 'fields=0x1;x0=-inf:1': 'NaN or infinite',
        'fields=0x1;x0=1:1e39': 'infinite after rounding', 'fields=0x1;x0=-3.5e38:1': 'infinite after rounding',
        'fields=0x1;x0=2:1': 'ascending', 'fields=0x1;x0=1:1': 'ascending', 'fields=0x1;x0=1:1.000000001:2': 'ascending',
        'fields=0x1,ord=1;x0=1:2;y=5:5.0000000001': 'ascending',
        'rows=6,rpb=-1,' + ok: 'rays_per_block', 'rows=6,rpb=4,' + ok: 'rays_per_block',
        'phase=0,' + ok: 'no pass open', 'phase=2,' + ok: 'no pass open',
        'counts=0,' + ok: 'counts',
    }
    for call, word in cases.items():
        line, = run(exe, call)
        assert line.startswith('refused ') and word in line, (call, line)
    # float64 keeps what float32 collapses; FLT_MAX itself is an edge
    assert run(exe, 'fields=0x200;x9=1:1.000000001:2')[0].startswith('ok ')
    assert run(exe, 'fields=0x200;x9=1:1e39')[0].startswith('ok ')
    assert run(exe, 'fields=0x1;x0=1:0x1.fffffep+127')[0].startswith('ok ')
    assert run(exe, 'fields=0x1,counts=0,phase=1;x0=1:2')[0].startswith('ok ')      # no counts needed before the finish


def test_host_header_pass(exe):
    a = 'rows=4,fields=0x3,ord=1,phase=%d;x0=1:2:3;x1=1:2;y=0:10'
    out = run(exe, a % 1, a % 0, 'gates=9,rows=11,fields=0x3,ord=1,phase=0;x0=1:2:3;x1=1:2;y=0:10', a % 2, a % 0)
    assert [parse(l)['open'] for l in out[:4]] == [1, 1, 1, 0] and out[4].startswith('refused') and 'no pass open' in out[4]
    # what differs from the open pass is refused and leaves it open: the call after it still finishes
    for other in ('rows=4,fields=0x1,ord=1,phase=0;x0=1:2:3;y=0:10',                  # fields
                  'rows=4,fields=0x3,ord=2,phase=0;x0=1:2:3;x1=1:2;y=0:10',            # ordinate
                  'rows=4,fields=0x3,ord=1,phase=0;x0=1:2:4;x1=1:2;y=0:10',            # an edge
                  'rows=4,fields=0x3,ord=1,phase=0;x0=1:2:3.0000001;x1=1:2;y=0:10',    # an edge that rounds to the same float32: accepted
                  'rows=4,fields=0x3,ord=1,phase=0;x0=1:2:3;x1=1:2;y=0:11',            # an ordinate edge
                  'rows=4,rpb=2,fields=0x3,ord=1,phase=0;x0=1:2:3;x1=1:2;y=0:10',      # blocks
                  'rows=4,fields=0x3,ord=1,phase=7;x0=1:2:3;x1=1:2;y=0:10'):           # any refusal
        out = run(exe, a % 1, other, a % 2)
        accepted = '3.0000001' in other
        assert out[1].startswith('ok ' if accepted else 'refused '), (other, out[1])
        assert parse(out[2])['open'] == 0 and parse(out[0])['open'] == 1
    # with blocks every call gives the same number of them, whatever its rows
    b = 'rows=%d,rpb=%d,fields=0x1,phase=%d;x0=1:2'
    out = run(exe, b % (6, 2, 1), b % (9, 3, 0), b % (8, 2, 0), b % (6, 2, 2))
    assert out[0].startswith('ok') and out[1].startswith('ok') and 'differ' in out[2] and parse(out[3])['open'] == 0
    # a begin in the middle starts over
    out = run(exe, a % 1, 'fields=0x4,phase=1;x2=1:2', 'fields=0x4,phase=2;x2=1:2')
    assert all(l.startswith('ok') for l in out)
