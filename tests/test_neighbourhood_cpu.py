"""Neighbourhood verification without a GPU: the rule (cosmo_pol_amd/neighbourhood.py: `sums`) against a literal loop over the
windows, the host helpers on hand-made cases, every ValueError of the spec, the product object `Scores` as
tests/test_products_cpu.py checks the others, the ctypes mirror of cpol_fractions against the header, and the host validation
header (cosmo_pol_amd/csrc/cpol_frac.h) through tests/c_host/frac_check.cpp, built with the address and undefined-behaviour
sanitizers and run as a program of its own.  All comparisons of sums are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import neighbourhood as NB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f4, u1, u8 = np.float32, np.uint8, np.uint64
nan, inf = np.nan, np.inf
SUMS = ('diff2', 'forecast2', 'observed2')
TOTALS = ('n_forecast', 'n_observed', 'n_domain')


def comp(n_x, n_y, fields=('ZH',), **kw):
    return CP.Composite(list(fields), np.arange(n_x + 1.0), np.arange(n_y + 1.0), **kw)


def frac(n_x, n_y, thresholds, radii, **kw):
    return NB.Fractions(comp(n_x, n_y), 'ZH', thresholds, radii, **kw)


# ---------------------------------------------------------------------------------------------------- the literal loop
def loop(spec, maps, obs, dom):
    nb, n_y, n_x = maps.shape
    thr, radii = spec.thresholds, [int(r) for r in spec.radii]
    s = np.zeros((nb, len(thr), len(radii), 3), dtype=object)
    t = np.zeros((nb, len(thr), 3), dtype=object)
    for b in range(nb):
        for it, th in enumerate(thr):
            F = [[bool(dom[y, x]) and maps[b, y, x] == maps[b, y, x] and maps[b, y, x] >= th for x in range(n_x)] for y in range(n_y)]
            Ob = [[bool(dom[y, x]) and obs[y, x] == obs[y, x] and obs[y, x] >= th for x in range(n_x)] for y in range(n_y)]
            t[b, it] = [sum(map(sum, F)), sum(map(sum, Ob)), int(np.count_nonzero(dom))]
            for w, r in enumerate(radii):
                for y in range(n_y):
                    for x in range(n_x):
                        if not dom[y, x]:
                            continue
                        nf = no = 0
                        for yy in range(y - r, y + r + 1):
                            for xx in range(x - r, x + r + 1):
                                if 0 <= yy < n_y and 0 <= xx < n_x:
                                    nf += F[yy][xx]
                                    no += Ob[yy][xx]
                        s[b, it, w] += [(nf - no) ** 2, nf * nf, no * no]
    return s.astype(u8), t.astype(u8)


def test_rule_against_the_literal_loop():
    rng = np.random.default_rng(5)
    pool = np.array([nan, -inf, inf, 0.0, -0.0, 0.5, 1.0, 1.0, 2.0, 3.5, 1e-42], dtype=f4)
    maps = pool[rng.integers(0, len(pool), (2, 5, 7))]
    obs = pool[rng.integers(0, len(pool), (5, 7))]
    dom = (rng.random((5, 7)) < 0.8).astype(u1)
    spec = frac(7, 5, [1.0, -inf, 3.0, inf], [0, 1, 2, 3, 9])
    for d in (None, dom):
        got = NB.sums(spec, maps, obs, d)
        s, t = loop(spec, maps, obs, np.ones((5, 7), u1) if d is None else d)
        assert s.any()
        for i, k in enumerate(SUMS):
            assert got[k].dtype == u8 and got[k].shape == (2, 4, 5) and np.array_equal(got[k], s[..., i]), k
        for i, k in enumerate(TOTALS):
            assert got[k].dtype == u8 and got[k].shape == (2, 4) and np.array_equal(got[k], t[..., i]), k
        assert got['radii'] is spec.radii and got['thresholds'] is spec.thresholds
    # a single map without the block axis, a bool domain; float64 maps are refused, not converted
    one = NB.sums(spec, maps[1], obs, dom.astype(bool))
    assert np.array_equal(one['diff2'], got['diff2'][1:])
    for bad in (lambda: NB.sums(spec, maps.astype(np.float64), obs), lambda: NB.sums(spec, maps, obs.astype(np.float64)),
                lambda: NB.sums(spec, maps[:, :4], obs), lambda: NB.sums(spec, maps, obs[:4]),
                lambda: NB.sums(spec, maps, obs, dom.astype(np.int32)), lambda: NB.sums(spec, maps, obs, dom[:, :3])):
        with pytest.raises(ValueError):
            bad()


def test_thresholds_are_compared_in_float32():
    # 0.1 rounds UP to float32: a float32 map value 0.1f reaches the threshold only when the threshold was rounded too
    spec = frac(1, 1, [0.1], [0])
    assert spec.thresholds.dtype == f4 and spec.thresholds_given[0] == 0.1
    assert NB.sums(spec, np.full((1, 1, 1), 0.1, f4), np.zeros((1, 1), f4))['n_forecast'][0, 0] == 1
    big = frac(1, 1, [1e39, -1e39], [0])          # beyond float32: +inf and -inf, allowed
    assert np.array_equal(big.thresholds, np.array([inf, -inf], f4))


# ---------------------------------------------------------------------------------------------------- the host helpers
def test_fss_identical_disjoint_and_empty():
    spec = frac(6, 4, [1.0], [0, 1, 2])
    a = np.zeros((1, 4, 6), f4)
    a[0, 1, 1] = a[0, 2, 4] = 5.0
    same = NB.sums(spec, a, a[0])
    assert same['diff2'].sum() == 0 and np.array_equal(NB.fss(same), np.ones((1, 1, 3)))
    b = np.zeros((4, 6), f4)
    b[0, 5] = b[3, 0] = 5.0                       # nowhere where `a` is set
    apart = NB.sums(spec, a, b)
    score = NB.fss(apart)
    assert score[0, 0, 0] == 0.0 and 0.0 < score[0, 0, 1] < score[0, 0, 2] < 1.0
    assert np.array_equal(NB.bias(apart), [[1.0]])
    none = NB.sums(spec, np.full((1, 4, 6), nan, f4), np.zeros((4, 6), f4))
    assert np.isnan(NB.fss(none)).all() and NB.fss(none).dtype == np.float64 and np.isnan(NB.bias(none)).all()


def test_contingency_against_boolean_counts():
    rng = np.random.default_rng(8)
    m = rng.random((3, 9, 11)).astype(f4)
    o = rng.random((9, 11)).astype(f4)
    m[0, 2, 3] = o[4, 4] = nan
    dom = (rng.random((9, 11)) < 0.7).astype(u1)
    spec = frac(11, 9, [0.3, 0.8], [0, 2])
    res = NB.sums(spec, m, o, dom)
    c = NB.contingency(res)
    d = dom != 0
    for b in range(3):
        for t, th in enumerate(spec.thresholds):
            F, O = d & (m[b] >= th), d & (o >= th)
            want = {'hits': (F & O).sum(), 'misses': (~F & O).sum(), 'false_alarms': (F & ~O).sum(),
                    'correct_negatives': (d & ~F & ~O).sum()}
            assert {k: int(c[k][b, t]) for k in c} == want
    assert all(c[k].dtype == u8 for k in c)
    with pytest.raises(ValueError, match='radius-0'):
        NB.contingency(NB.sums(frac(11, 9, [0.3], [1, 2]), m, o))


# ---------------------------------------------------------------------------------------------------- the spec
def test_spec_refusals_and_identity():
    c = comp(4, 3, fields=('ZH', 'KDP'), products=('max', 'echo_top'), thresholds=[1.0, 2.0])
    ok = NB.Fractions(c, 'KDP', [1.0], [0, 5], plane='echo_top_1')
    assert (ok.plane_index, ok.n_x, ok.n_y) == (3, 4, 3) and ok.radii.dtype == np.int32
    assert NB.Fractions(c, 'ZH', [1.0], [1.0, 2.0]).radii.tolist() == [1, 2]        # integral floats are integers
    for args, kw, what in (
            (('nope', 'ZH', [1.0], [0]), {}, 'composite_spec'),
            ((c, 'RVEL', [1.0], [0]), {}, 'RVEL'),
            ((c, 'ZV', [1.0], [0]), {}, 'not a field'),
            ((c, 'ZH', [1.0], [0]), {'plane': 'lowest'}, 'not a plane'),
            ((c, 'ZH', [1.0], [0]), {'plane': 'echo_top_2'}, 'not a plane'),
            ((c, 'ZH', [], [0]), {}, 'thresholds: 1 ... 4'),
            ((c, 'ZH', [1, 2, 3, 4, 5], [0]), {}, 'thresholds: 1 ... 4'),
            ((c, 'ZH', [1.0, nan], [0]), {}, 'NaN'),
            ((c, 'ZH', [1.0], []), {}, 'radii: 1 ... 8'),
            ((c, 'ZH', [1.0], list(range(9))), {}, 'radii: 1 ... 8'),
            ((c, 'ZH', [1.0], [-1, 2]), {}, 'outside 0 ... 1023'),
            ((c, 'ZH', [1.0], [3, 1024]), {}, 'outside 0 ... 1023'),
            ((c, 'ZH', [1.0], [1, 1]), {}, 'strictly ascending'),
            ((c, 'ZH', [1.0], [2, 1]), {}, 'strictly ascending'),
            ((c, 'ZH', [1.0], [1.5]), {}, 'integers'),
            ((c, 'ZH', [1.0], [nan]), {}, 'integers')):
        with pytest.raises(ValueError, match=what):
            NB.Fractions(*args, **kw)
    NB.Fractions(c, 'ZH', [-inf, inf], [0, 1023])
    a, b = NB.Fractions(c, 'ZH', [0.1], [1, 2]), NB.Fractions(c, 'ZH', [np.float32(0.1)], (1, 2))
    assert a == b and hash(a) == hash(b) and a.key == b.key          # (the ROUNDED thresholds identify a spec)
    assert a != NB.Fractions(c, 'ZH', [0.1], [1, 3]) and a != NB.Fractions(c, 'KDP', [0.1], [1, 2]) and a != 'a'
    assert a != NB.Fractions(c, 'ZH', [0.1], [1, 2], plane='height_of_max')
    assert a != NB.Fractions(comp(4, 4, fields=('ZH',)), 'ZH', [0.1], [1, 2])
    assert repr(a).startswith('Fractions(ZH max of Composite(') and 'radii=[1, 2]' in repr(a)
    assert NB.scratch_bytes(a, 2) == 3 * 1 * 4 * 5 * 4


# ---------------------------------------------------------------------------------------------------- the product object
def attach(product, az, n_gates, n_members=None, take=None):
    structs, keep = product.attach(N, az, n_gates, n_members, True, True, ['U', 'V', 'W', 'T'], take)
    for slot in structs:
        assert slot in dict(N.Outputs._fields_)
    return structs


def test_scores_arrays_binding_finish_join():
    c = CP.Composite(['KDP', 'ZH'], [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0], products=('max', 'lowest'))      # a 2 x 3 grid
    spec = NB.Fractions(c, 'KDP', [0.5, 1.5], [0, 1, 4], plane='lowest')
    obs = np.arange(6, dtype=f4).reshape(2, 3)
    dom = np.array([[1, 0, 1], [1, 1, 0]], u1)
    p = NB.Scores(spec, obs, dom, keep_gates=False, phase=3, rays_per_block=2)
    assert (p.name, p.gates, p.spectrum, p.model_var) == ('composite', False, True, None) and p.refuses is CP.Maps.refuses
    assert NB.Scores(spec, obs, keep_gates=True).gates
    taken = []

    def take(block):
        views = [np.zeros(sh, dt) for _, dt, sh in block]
        taken.append((block, views))
        return views, [0x77000 + 64 * i for i in range(len(block))]
    az4 = np.arange(4.0)
    structs = attach(p, az4, 5, take=take)
    assert sorted(structs) == ['composite', 'fractions']
    cs, f = structs['composite'], structs['fractions']
    assert (cs.fields, cs.phase, cs.rays_per_block, cs.n_x, cs.n_y) == (0b1001, 3, 2, 3, 2)
    assert (f.field, f.plane, f.n_thresholds, f.n_radii) == (3, 2, 2, 3)
    assert list(f.thresholds)[:2] == [0.5, 1.5] and list(f.radii)[:3] == [0, 1, 4]
    # the observed map and the domain: a clean block of their own, written before the call, bound to their slots
    assert taken[0][0] == [('observed', f4, (2, 3)), ('domain', u1, (2, 3))]
    assert (taken[0][1][0] == obs).all() and (taken[0][1][1] == dom).all()
    assert (f.observed, f.domain) == (0x77000, 0x77040)
    assert p.arrays() == [('ZH', f4, (2, 4, 2, 3)), ('KDP', f4, (2, 4, 2, 3)), ('count', u8, (2, 2, 2, 3)),
                          ('sums', u8, (2, 2, 3, 3)), ('totals', u8, (2, 2, 3))]
    bound = {}
    for i, (path, _, _) in enumerate(p.arrays()):
        bound[path] = 0x1000 * (i + 1)
        p.bind(path, bound[path])
    assert [x or 0 for x in cs.values] == [bound.get(k, 0) for k in CP.FIELDS] and cs.count == bound['count']
    assert (f.sums, f.totals) == (bound['sums'], bound['totals'])
    # without a domain: one array in the block, the slot NULL; an ensemble call: a block per member
    q = NB.Scores(spec, obs, None, rays_per_block=4)
    f = attach(q, az4, 5, n_members=3, take=take)['fractions']
    assert taken[1][0] == [('observed', f4, (2, 3))] and not f.domain
    assert q.arrays()[-2:] == [('sums', u8, (3, 2, 3, 3)), ('totals', u8, (3, 2, 3))]
    # device outputs: no `take`; the composite's entries and the four of the scores are accepted, any other refused
    d = NB.Scores(spec)
    structs = attach(d, az4, 5)
    f, cs = structs['fractions'], structs['composite']
    d.bind_device({'values': {'KDP': 5}, 'count': 6, 'observed': 7, 'domain': 8, 'sums': 9, 'totals': 10})
    assert (f.observed, f.domain, f.sums, f.totals, cs.count, cs.values[3]) == (7, 8, 9, 10, 6, 5)
    with pytest.raises(ValueError, match="unknown entry 'ZH'"):
        d.bind_device({'ZH': 1})
    with pytest.raises(ValueError, match='needs the observed map'):
        attach(NB.Scores(spec), az4, 5, take=take)
    # a call that does not finish the pass: the composite's struct alone, no arrays, no block, no entry read
    p.phase = 1
    n_taken = len(taken)
    structs = attach(p, az4, 5, take=take)
    assert sorted(structs) == ['composite'] and structs['composite'].phase == 1 and p.arrays() == [] and len(taken) == n_taken
    p.bind_device({'sums': 1, 'nonsense': 2})
    # what the constructor and the attach refuse: those of Maps
    with pytest.raises(ValueError, match='spec: a cosmo_pol_amd.neighbourhood.Fractions'):
        NB.Scores(c, obs)
    with pytest.raises(NotImplementedError, match='process group'):
        NB.Scores(spec, obs, distributed=True)
    with pytest.raises(ValueError, match='does not divide the 8 rows'):
        attach(NB.Scores(spec, obs, rays_per_block=3), az4, 5, n_members=2, take=take)
    big = NB.Fractions(comp(1023, 1023), 'ZH', [1, 2, 3, 4], [0])
    with pytest.raises(ValueError, match='more than 1 GiB'):
        attach(NB.Scores(big, np.zeros((1023, 1023), f4), rays_per_block=1), np.arange(64.0), 5, take=take)
    # the finish: the composite's result with one more key; the join: blocks on the leading axis
    p.phase = 3
    attach(p, az4, 5, take=take)
    views = {path: np.zeros(sh, dt) for path, dt, sh in p.arrays()}
    views['sums'] = np.arange(3, dtype=u8)[None, None, None, :] * np.ones((2, 2, 3, 3), u8)
    views['totals'] = (10 + np.arange(3, dtype=u8))[None, None, :] * np.ones((2, 2, 3), u8)
    out = p.finish(views, None)
    assert sorted(out) == ['count', 'fractions', 'values', 'x_edges', 'y_edges']
    fr = out['fractions']
    assert sorted(fr) == sorted(SUMS + TOTALS + ('thresholds', 'radii')) and fr['radii'] is spec.radii
    assert all(fr[k].shape == (2, 2, 3) and (fr[k] == i).all() for i, k in enumerate(SUMS))
    assert all(fr[k].shape == (2, 2) and (fr[k] == 10 + i).all() for i, k in enumerate(TOTALS))
    j = p.join([out, out], np.concatenate)
    assert j['fractions']['diff2'].shape == (4, 2, 3) and j['fractions']['n_domain'].shape == (4, 2)
    assert j['values']['KDP']['lowest'].shape == (4, 2, 3) and j['fractions']['thresholds'] is spec.thresholds
    p.rays_per_block = 0
    assert p.join([None, out], np.concatenate)['fractions'] is fr


def test_scores_block_through_the_packer():
    """The observed map and the uint8 domain through the operator's own block packer (one byte per cell, 64-byte aligned)."""
    class Pool(object):
        def take(self, nbytes, writer=None):
            return np.zeros(nbytes + 64, np.uint8), {'ctx': None, 'serial': 0}
    spec = frac(3, 2, [0.5], [0, 1])
    obs, dom = np.arange(6, dtype=f4).reshape(2, 3), np.array([[1, 0, 1], [0, 1, 1]], u1)
    p = NB.Scores(spec, obs, dom)
    blocks = []

    def take(block):
        views, addresses, _ = N.carve_block(Pool(), block)
        blocks.append((views, addresses))
        return views, addresses
    f = attach(p, np.arange(4.0), 5, take=take)['fractions']
    (views, addresses), = blocks
    assert (f.observed, f.domain) == tuple(addresses) and addresses[1] - addresses[0] == 64
    assert views[1].dtype == u1 and np.array_equal(views[0], obs) and np.array_equal(views[1], dom)
    views, addresses, _ = N.carve_block(Pool(), p.arrays())
    assert [v.shape for v in views[-2:]] == [(1, 1, 2, 3), (1, 1, 3)] and views[-1].dtype == u8


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_struct_layout_matches_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){',
             'printf("cpol_fractions %zu\\n", sizeof(cpol_fractions));']
    for fname, _ in N.Fractions._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(cpol_fractions, %s));' % (fname, fname))
    lines.append('printf("slot %zu\\n", offsetof(cpol_outputs, fractions));')
    lines.append('printf("limits %d %d %d\\n", CPOL_FRAC_MAX_THRESHOLDS, CPOL_FRAC_MAX_RADII, CPOL_FRAC_MAX_RADIUS);')
    lines.append('cpol_outputs o; memset(&o, 0, sizeof o); printf("off %d\\n", o.fractions == NULL); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got['cpol_fractions']) == C.sizeof(N.Fractions)
    for fname, _ in N.Fractions._fields_:
        assert int(got[fname]) == getattr(N.Fractions, fname).offset, fname
    assert int(got['slot']) == N.Outputs.fractions.offset and got['off'] == '1' and not N.Outputs().fractions
    assert got['limits'].split() == [str(NB.MAX_THRESHOLDS), str(NB.MAX_RADII), str(NB.MAX_RADIUS)]
    # in front of the members that earlier tests pin where they are
    names = [f for f, _ in N.Outputs._fields_]
    assert names[names.index('sz_total') - 1] == 'fractions' and names[names.index('fractions') - 1] == 'model_vars'
    spec = NB.Fractions(comp(4, 3, fields=('ZV', 'ATT_V')), 'ATT_V', [0.1, 1e39], [0, 7], plane='height_of_max')
    f, keep = N.Context.fractions_struct(spec)
    assert (f.field, f.plane, f.n_thresholds, f.n_radii) == (8, 1, 2, 2)
    assert list(f.thresholds) == [0.1, 1e39, 0.0, 0.0] and list(f.radii) == [0, 7, 0, 0, 0, 0, 0, 0]        # (the library rounds)
    assert not f.observed and not f.domain and not f.sums and not f.totals


# ---------------------------------------------------------------------------------------------------- the host validation header
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('frac') / 'frac_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'frac_check.cpp'),
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
    head, thr, radii = line.split(' | ')
    w = head.split()
    out = {name: int(x) for name, x in zip(w[1::2], w[2::2])}
    out['thr'] = [float.fromhex(x) if 'x' in x else float(x) for x in thr.split()[1:]]
    out['radii'] = [int(x) for x in radii.split()[1:]]
    return out


def test_host_check_accepts_and_plans(exe):
    # a 3 x 2 grid, one block; field 0, products MAX: planes max, height_of_max
    got = parse(run(exe, 'plane=1;t=0.1:-inf:1e39;r=0:3:1023')[0])
    assert got['thr'] == [float(f4(0.1)), -inf, inf] and got['radii'] == [0, 3, 1023]
    assert (got['blocks'], got['cells'], got['table'], got['tables'], got['scratch']) == (1, 6, 12, 6, 6 * 12 * 4)
    assert (got['field'], got['first'], got['stride']) == (0, 6, 12)
    assert (got['rows'], got['cols'], got['score'], got['chunks'], got['groups']) == (2 * 1, 6 * 1, 3 * 1, 1, 1)
    assert (got['sums'], got['totals']) == (1 * 3 * 3 * 3 * 8, 1 * 3 * 3 * 8)
    # fields ZH and KDP with MAX | LOWEST | ECHO_TOP (two thresholds): six planes; four blocks of one ray; a 130 x 67 grid
    got = parse(run(exe, 'cfields=0x9,cproducts=7,ctop=2,field=3,plane=5,rows=4,rpb=1,nx=130,ny=67,dom=1;t=1;r=2')[0])
    assert (got['blocks'], got['cells'], got['table'], got['tables']) == (4, 8710, 68 * 131, 5)
    assert (got['field'], got['first'], got['stride']) == (3, 5 * 8710, 6 * 8710)
    assert (got['rows'], got['cols'], got['score'], got['chunks'], got['groups']) == (5 * 17, 5 * 3, 4 * 9, 3, 9)
    # the largest grid; the cap on the tables is met exactly by 63 blocks and four thresholds, and missed by 64
    got = parse(run(exe, 'nx=1023,ny=1023,rows=63,rpb=1;t=1:2:3:4;r=0:1:2:3:4:5:6:7')[0])
    assert got['scratch'] == 1 << 30 and got['groups'] == 1023 and got['score'] == 63 * 4 * 1023
    assert run(exe, 'nx=1023,ny=1023,rows=64,rpb=1;t=1:2:3:4;r=0')[0] == \
        'refused the summed-area tables of all blocks and thresholds must be at most 1 GiB'
    assert run(exe, 'nx=1023,ny=1023,rows=64,rpb=1;t=1:2:3;r=0')[0].startswith('ok ')


def test_host_check_refusals(exe):
    cases = [
        ('comp=0;t=1;r=0', 'needs a composite'),
        ('cphase=1;t=1;r=0', 'does not finish its pass'),
        ('cphase=0;t=1;r=0', 'composite refused'),                      # (no pass open: the composite's own refusal comes first)
        ('field=1;t=1;r=0', 'field is not among the composed fields'),
        ('field=-1;t=1;r=0', 'field is not among the composed fields'),
        ('field=9;t=1;r=0', 'field is not among the composed fields'),
        ('field=31;t=1;r=0', 'field is not among the composed fields'),
        ('plane=2;t=1;r=0', 'plane lies outside'),
        ('plane=-1;t=1;r=0', 'plane lies outside'),
        ('cproducts=7,ctop=1,plane=5;t=1;r=0', 'plane lies outside'),
        (';r=0', 'n_thresholds must lie in 1 ... 4'),
        ('nthr=5;t=1:2:3:4;r=0', 'n_thresholds must lie in 1 ... 4'),
        ('nthr=-1;t=1;r=0', 'n_thresholds must lie in 1 ... 4'),
        (';t=1:nan;r=0', 'a threshold is NaN'),
        (';t=1', 'n_radii must lie in 1 ... 8'),
        ('nrad=9;t=1;r=0:1:2:3:4:5:6:7', 'n_radii must lie in 1 ... 8'),
        (';t=1;r=-1', 'a radius must lie in 0 ... 1023'),
        (';t=1;r=0:1024', 'a radius must lie in 0 ... 1023'),
        (';t=1;r=1:1', 'strictly ascending'),
        (';t=1;r=3:2', 'strictly ascending'),
        ('obs=0;t=1;r=0', 'observed is NULL'),
        ('sums=0;t=1;r=0', 'sums or totals is NULL'),
        ('totals=0;t=1;r=0', 'sums or totals is NULL'),
    ]
    for line, (_, want) in zip(run(exe, *[c for c, _ in cases]), cases):
        assert line.startswith('composite refused' if want == 'composite refused' else 'refused ') and want in line, (line, want)
    # what is allowed: both infinities, radius 0 alone and 1023, a radius wider than the grid, eight radii, no domain
    for line in run(exe, ';t=-inf:inf;r=0', ';t=1;r=1023', ';t=1;r=0:1:2:3:4:5:6:1023', 'cproducts=7,ctop=4,plane=7;t=1;r=0'):
        assert line.startswith('ok '), line
