"""Ensemble quantiles without a GPU: the rule of ensemble_stats (EnsembleQuantiles; `quantiles`, fold / finish / reduce) against
np.nanquantile and against a plain-Python loop written here from the rule's text, its invariances (member order, cuts of the
pass), the edge cases, the refusals, and the layout of the members appended to cpol_member_stats against the header."""
import ast
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import ensemble_stats as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = [0.0, 1.0, 0.5, 0.1, 0.9, 1.0 / 3.0, 0.25]
ORDER = ('lower', 'higher', 'nearest')


def members(M, n_cells=400, seed=0, nan=0.2, dtype=np.float32):
    """standard-normal members, 20 % NaN, cell 0 all NaN"""
    rng = np.random.default_rng(seed + M)
    x = rng.standard_normal((M, n_cells)).astype(dtype)
    x[rng.random(x.shape) < nan] = np.nan
    x[:, 0] = np.nan
    return x


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def nanquantile(x, q, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # (all-NaN cells: NaN is what we want there)
        return np.nanquantile(x, q, axis=0, **kw)


def before(a, b):
    """the rule's order: <, and -0.0 before +0.0"""
    return bool(a < b or (a == b and np.signbit(a) and not np.signbit(b)))


def loop_quantiles(x, q, method, need):
    """The rule, cell by cell, in Python floats (IEEE float64) and NumPy scalars of the field's type."""
    T = x.dtype.type
    out = np.full((len(q), x.shape[1]), np.nan, T)
    for c in range(x.shape[1]):
        s = []
        for v in x[:, c]:
            if v == v:
                j = len(s)
                while j > 0 and before(v, s[j - 1]):
                    j -= 1
                s.insert(j, v)
        n = len(s)
        if n < need or n == 0:
            continue
        for t, qt in enumerate(q):
            h = float(np.float64(qt) * np.float64(n - 1))
            i = int(np.floor(h))
            if method == 'linear':
                g = h - float(i)
                a = np.float64(s[i])
                r = s[i]
                if g != 0.0:
                    b = np.float64(s[i + 1])
                    if a != b:
                        with np.errstate(all='ignore'):
                            r64 = a + np.float64(g) * (b - a)
                            if r64 > b:
                                r64 = b
                            r = T(r64)
            elif method == 'lower':
                r = s[i]
            elif method == 'higher':
                r = s[int(np.ceil(h))]
            else:
                r = s[int(np.rint(h))]
            out[t, c] = r
    return out


@pytest.mark.parametrize('T', [np.float32, np.float64])
@pytest.mark.parametrize('M', [1, 2, 3, 5, 21, 64, 128])
def test_rule_against_numpy(M, T):
    """Measured here (standard-normal members, 400 cells, 20 % NaN): lower / higher / nearest equal np.nanquantile exactly;
    linear on float64 deviates by at most 3.6e-16 of the cell's largest magnitude (bound 1e-13, the mean's); linear on float32
    is within one float32 unit in the last place of np.nanquantile of the float64-cast members rounded to float32."""
    x = members(M, dtype=T)
    for method in ORDER:
        got = ES.quantiles(x, QS, method)
        assert got.dtype == T and same_bits(got, nanquantile(x, QS, method=method).astype(T)), method
    got = ES.quantiles(x, QS, 'linear')
    ref64 = nanquantile(x.astype(np.float64), QS)
    assert got.dtype == T and got.shape == ref64.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref64)) and np.isnan(got[:, 0]).all()
    ok = ~np.isnan(ref64)
    if T == np.float64:
        big = np.nanmax(np.abs(x), axis=0, initial=0.0)[None] * np.ones_like(ref64)
        e = np.max(np.abs(got[ok] - ref64[ok]) / big[ok]) if ok.any() else 0.0
        print('M = %d float64 linear: %.3g of the largest magnitude' % (M, e))
        assert e <= 1e-13
    else:
        ref = ref64.astype(np.float32)
        ulp = np.spacing(np.maximum(np.abs(ref), np.abs(got)))
        e = np.max(np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64)) / ulp[ok]) if ok.any() else 0.0
        print('M = %d float32 linear: %.3g ulp' % (M, e))
        assert e <= 1.0
    # through begin / fold / finish, with the other statistics unchanged beside them
    name = 'RVEL' if T == np.float64 else 'ZH'
    spec = ES.EnsembleQuantiles({name: QS}, fields=[name], extremes=True)
    res = ES.reduce({name: x}, spec)
    plain = ES.reduce({name: x}, ES.EnsembleStats(fields=[name], extremes=True))
    assert set(res) == set(plain) | {'quantile'} and set(res['quantile']) == {name}
    assert same_bits(res['quantile'][name], got)
    for kind in ('mean', 'spread', 'min', 'max', 'count'):
        assert np.array_equal(res[kind][name], plain[kind][name], equal_nan=True), kind


@pytest.mark.parametrize('T', [np.float32, np.float64])
@pytest.mark.parametrize('method', ES.METHODS)
def test_rule_is_the_python_loop(method, T):
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((9, 60)) * 10.0 ** rng.integers(-4, 5, (9, 60))).astype(T)
    x[:, 40:50] = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), (9, 10)).astype(T)
    x[:, 50:] = rng.choice(np.array([-np.inf, np.inf, 2.0, 3.0, -0.0]), (9, 10)).astype(T)
    x[rng.random(x.shape) < 0.25] = np.nan
    x[:, 0] = np.nan
    x[1:, 1] = np.nan
    q = [0.0, 1.0, 0.5, 0.125, 1.0 / 3.0, 0.9, 0.75, 0.25]
    for need in (1, 3):
        with np.errstate(all='ignore'):
            got = ES.quantiles(x, q, method, need)
        assert same_bits(got, loop_quantiles(x, q, method, need)), (method, need)


def test_permutations_and_cuts_give_the_same_bits():
    rng = np.random.default_rng(2)
    M = 21
    rows = {'ZH': members(M, 300), 'RVEL': members(M, 300, seed=9, dtype=np.float64) * 7.0 - 10.0}
    rows['ZH'][:, 5:40] = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], np.float32), (M, 35))
    for method in ES.METHODS:
        spec = ES.EnsembleQuantiles({'ZH': QS, 'RVEL': [0.5, 0.9]}, method=method, min_members=2)
        whole = ES.reduce(rows, spec)
        assert whole['quantile']['ZH'].shape == (len(QS), 300) and whole['quantile']['RVEL'].dtype == np.float64
        for _ in range(3):
            p = rng.permutation(M)
            other = ES.reduce({k: v[p] for k, v in rows.items()}, spec)
            for k in rows:
                assert same_bits(other['quantile'][k], whole['quantile'][k]), (method, k)
        for cut in ([1] * M, [M - 1, 1], [1, M - 1], [11, 10], [0, M, 0]):
            st = ES.begin(spec, ['ZH', 'RVEL'], (300,))
            at = 0
            for n in cut:
                ES.fold(st, {k: v[at:at + n] for k, v in rows.items()})
                at += n
            assert st['fields']['ZH']['x'].shape == (M, 300) and same_bits(st['fields']['ZH']['x'], rows['ZH'])
            res = ES.finish(st, spec)
            for kind in whole:
                if kind != 'n_members':
                    for k in whole[kind]:
                        assert same_bits(res[kind][k], whole[kind][k]), (method, cut, kind, k)


def test_edge_cases():
    nan, inf = np.nan, np.inf
    f = np.float32
    x = np.array([[nan, 1.0, nan, 2.5, 2.0, 0.0, -0.0, inf, -inf, 1.0, 5.0],
                  [nan, nan, nan, 2.5, 3.0, -0.0, 0.0, 1.0, -inf, nan, 5.0],
                  [nan, nan, 4.0, 2.5, 2.0, 0.0, -0.0, 2.0, 1.0, 3.0, -5.0]], dtype=f)
    for method in ES.METHODS:
        spec = ES.EnsembleQuantiles({'ZH': [0.0, 0.5, 1.0]}, method=method, extremes=True, min_members=2)
        r = ES.reduce({'ZH': x}, spec)
        q = r['quantile']['ZH']
        # below need: NaN, like the mean; all NaN: NaN
        assert np.isnan(q[:, :3]).all() and np.isnan(r['mean']['ZH'][:3]).all(), method
        # duplicates and all-equal cells give that value
        assert (q[:, 3] == f(2.5)).all() and q[1, 4] == 2.0 and q[1, 10] == 5.0
        # q = 0 and q = 1 are min and max (values; the sign of a zero is the ordering's, see below)
        assert np.array_equal(q[0], r['min']['ZH'], equal_nan=True) and np.array_equal(q[2], r['max']['ZH'], equal_nan=True)
        # -0.0 before +0.0: the lowest of {+0, -0, +0} is -0.0 and the highest +0.0, whatever the order they came in, while min
        # and max keep the first zero met
        for c in (5, 6):
            assert q[0, c] == 0.0 and np.signbit(q[0, c]) and q[2, c] == 0.0 and not np.signbit(q[2, c]), (method, c)
        assert not np.signbit(r['min']['ZH'][5]) and np.signbit(r['max']['ZH'][6])
        assert np.signbit(q[1, 6]) and not np.signbit(q[1, 5])          # the medians of {-0, -0, +0} and {-0, +0, +0}
        # infinite members are ordered like any other value
        assert q[0, 7] == 1.0 and q[1, 7] == 2.0 and q[2, 7] == inf and q[0, 8] == -inf and q[2, 8] == 1.0 and q[1, 8] == -inf
    # linear between an infinite bracket: what IEEE gives
    lin = ES.quantiles(np.array([[-inf, 1.0, 1.0], [2.0, inf, inf]], dtype=f), [0.25, 0.5])
    assert np.isnan(lin[:, 0]).all() and (lin[:, 1:] == inf).all()
    assert np.isnan(ES.quantiles(np.array([[-inf], [inf]], dtype=f), [0.5])).all()
    assert ES.quantiles(np.array([[inf], [inf], [1.0]], dtype=f), [0.75])[0, 0] == inf         # (equal brackets: a, not inf - inf)
    # one member: every quantile is that member; need = 1 by default
    one = ES.quantiles(np.array([[3.0, nan]], dtype=f), [0.0, 0.3, 1.0], 'linear')
    assert (one[:, 0] == 3.0).all() and np.isnan(one[:, 1]).all()
    # no member at all
    assert np.isnan(ES.quantiles(np.zeros((0, 4), f), [0.5])).all()
    # the interpolation is clamped to its upper bracket and rounded once to the field's type
    a, b = f(1.0), np.nextafter(f(1.0), f(2.0))
    mid = ES.quantiles(np.array([[a], [b]], dtype=f), [0.5, 0.999999])
    assert a <= mid[0, 0] <= b and mid[1, 0] == b


@pytest.mark.parametrize('T', [np.float32, np.float64])
def test_db_commutes_with_the_order_statistics(T):
    rng = np.random.default_rng(4)
    x = (10.0 ** rng.uniform(-3, 6, (21, 300))).astype(T)
    x[rng.random(x.shape) < 0.2] = np.nan
    assert ES.db(x).dtype == T and ES.db(np.array([1.0, 10.0, 100.0], T)).tolist() == [0.0, 10.0, 20.0]
    assert ES.db([1, 1000]).tolist() == [0.0, 30.0] and 'lower' in ES.db.__doc__ and 'nearest' in ES.db.__doc__
    for method in ORDER:
        assert same_bits(ES.db(ES.quantiles(x, QS, method)), ES.quantiles(ES.db(x), QS, method)), method
    assert ES.dbz(35.0) == 10.0 ** 3.5


def test_refusals_and_the_spec():
    Q = ES.EnsembleQuantiles
    for kw in (dict(quantiles={'DSPECTRUM': [0.5]}), dict(quantiles={'ZV': [0.5]}, fields=['ZH']), dict(quantiles={'ZH': []}),
               dict(quantiles={'ZH': list(np.linspace(0, 1, 9))}), dict(quantiles={'ZH': [np.nan]}), dict(quantiles={'ZH': [-0.01]}),
               dict(quantiles={'ZH': [0.5, 1.01]}), dict(quantiles={'ZH': [[0.5]]}), dict(quantiles={'ZH': 0.5}, method='median'),
               dict(quantiles={'ZH': 0.5}, method=0), dict(quantiles=[0.5]), dict(quantiles={'ZH': 0.5}, min_members=0),
               dict(quantiles={'ZH': 0.5}, exceed={'ZH': [np.nan]})):
        with pytest.raises(ValueError):
            Q(**kw)
    spec = Q({'ZH': 0.5, 'RVEL': [0.1, 0.9]}, method='nearest', extremes=True, min_members=2)
    assert isinstance(spec, ES.EnsembleStats) and spec.quantiles['ZH'].shape == (1,) and spec.method == 'nearest'
    assert spec.extremes and spec.min_members == 2 and list(spec.quantiles['RVEL']) == [0.1, 0.9]
    assert Q({'ZH': list(np.linspace(0, 1, 8))}).quantiles['ZH'].size == 8
    with pytest.raises(ValueError):                         # RVEL without Doppler
        spec.resolve(['ZH', 'ZV'])
    assert spec.resolve(['ZH', 'RVEL', 'mask']) == ('ZH', 'RVEL')
    # key and repr carry the new terms
    assert spec.key != Q({'ZH': 0.5, 'RVEL': [0.1, 0.9]}, method='lower', extremes=True, min_members=2).key
    assert spec.key != Q({'ZH': 0.25, 'RVEL': [0.1, 0.9]}, method='nearest', extremes=True, min_members=2).key
    assert spec.key == Q({'RVEL': [0.1, 0.9], 'ZH': [0.5]}, method='nearest', extremes=True, min_members=2).key
    assert spec.key[:len(ES.EnsembleStats(extremes=True, min_members=2).key)] == ES.EnsembleStats(extremes=True, min_members=2).key
    assert 'nearest' in repr(spec) and '0.9' in repr(spec) and repr(spec).startswith('EnsembleQuantiles(')
    # median
    med = Q.median(['ZH', 'KDP'], method='lower', mean=False)
    assert set(med.quantiles) == {'ZH', 'KDP'} and list(med.quantiles['KDP']) == [0.5] and med.method == 'lower' and not med.mean
    assert set(Q.median(fields=['ZH', 'ZV']).quantiles) == {'ZH', 'ZV'} and 'RVEL' not in Q.median().quantiles
    with pytest.raises(ValueError):
        Q.median(['mask'])
    # fold past 128 members with quantiles; a plain spec goes on
    x = np.ones((ES.MAX_QUANTILE_MEMBERS, 3), np.float32)
    st = ES.fold(ES.begin(med, ['ZH', 'KDP'], (3,)), {'ZH': x, 'KDP': x})
    with pytest.raises(ValueError, match='128'):
        ES.fold(st, {'ZH': x[:1], 'KDP': x[:1]})
    with pytest.raises(ValueError, match='128'):
        ES.reduce({'ZH': np.ones((129, 3), np.float32)}, Q({'ZH': 0.5}))
    assert ES.finish(st)['quantile']['ZH'].tolist() == [[1.0, 1.0, 1.0]]
    plain = ES.fold(ES.fold(ES.begin(ES.EnsembleStats(), ['ZH'], (3,)), {'ZH': x}), {'ZH': x})
    assert plain['n_members'] == 256 and 'x' not in plain['fields']['ZH']
    assert ES.MAX_QUANTILES == 8 and ES.MAX_QUANTILE_MEMBERS == 128 and ES.METHODS == ('linear', 'lower', 'higher', 'nearest')


def test_a_plain_spec_is_unchanged():
    x = members(5, 50)
    res = ES.reduce({'ZH': x}, ES.EnsembleStats(extremes=True, exceed={'ZH': [0.0]}))
    assert set(res) == {'mean', 'spread', 'min', 'max', 'count', 'exceed', 'n_members'}
    # a field of a quantile spec without quantiles keeps no members
    st = ES.begin(ES.EnsembleQuantiles({'ZH': 0.5}), ['ZH', 'ZV'], (50,))
    assert 'x' in st['fields']['ZH'] and 'x' not in st['fields']['ZV']
    res = ES.finish(ES.fold(st, {'ZH': x, 'ZV': x}))
    assert set(res['quantile']) == {'ZH'} and set(res['mean']) == {'ZH', 'ZV'}


def test_struct_layout_matches_header(tmp_path):
    old = ['phase', 'min_members', 'fields', 'n_thresholds', 'thresholds', 'mean', 'spread', 'min', 'max', 'count', 'exceed']
    new = ['quantile_capacity', 'quantile_method', 'n_quantiles', 'quantiles', 'quantile']
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "cosmo_pol_amd.h"\nint main(void) {\n'
                   'cpol_member_stats m; memset(&m, 0, sizeof m);\n'
                   'printf("%zu %d %d %d\\n", sizeof(cpol_member_stats), m.quantile_capacity, m.n_quantiles[9], m.quantile[0] == NULL);\n'
                   + ''.join('printf("%%zu\\n", offsetof(cpol_member_stats, %s));\n' % n for n in old + new)
                   + 'printf("%zu %zu %zu %d %d\\n", sizeof(m.n_quantiles), sizeof(m.quantiles), sizeof(m.quantile),\n'
                   '       CPOL_MEMBER_STATS_MAX_QUANTILES, CPOL_MEMBER_STATS_MAX_QUANTILE_MEMBERS);\n'
                   'return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    M = N.MemberStats
    ptrs = ctypes.sizeof(ctypes.c_void_p) * 10
    assert got == ([ctypes.sizeof(M), 0, 0, 1] + [getattr(M, n).offset for n in old + new]
                   + [40, ptrs, ptrs, ES.MAX_QUANTILES, ES.MAX_QUANTILE_MEMBERS])
    # the old members where they were (LP64: three int32, ten int32, a pad, then pointers), the new ones behind them
    assert [getattr(M, n).offset for n in old] == [0, 4, 8, 12, 56, 136, 216, 296, 376, 456, 464]
    assert [n for n, _ in M._fields_[-5:]] == new and M.quantile_capacity.offset == M.exceed.offset + ptrs
    assert M.quantile.offset + ptrs == ctypes.sizeof(M)
    z = M()
    assert z.quantile_capacity == 0 and z.quantile_method == 0 and not any(z.n_quantiles) and not any(z.quantile)


def test_member_stats_struct_of_a_spec():
    spec = ES.EnsembleQuantiles({'ZH': [0.1, 0.5, 0.9], 'RVEL': 0.5}, method='higher', exceed={'ZH': [1.0]}, min_members=2)
    ms, keep = N.Context.member_stats_struct(spec, ('ZH', 'KDP', 'RVEL'), 3, capacity=21)
    assert ms.phase == 3 and ms.min_members == 2 and ms.fields == (1 << 0) | (1 << 3) | (1 << 9)
    assert ms.quantile_capacity == 21 and ms.quantile_method == 2
    assert list(ms.n_quantiles) == [3, 0, 0, 0, 0, 0, 0, 0, 0, 1] and list(ms.n_thresholds) == [1] + [0] * 9
    ptrs = {a.ctypes.data: a for a in keep}
    assert list(ptrs[ms.quantiles[0]]) == [0.1, 0.5, 0.9] and list(ptrs[ms.quantiles[9]]) == [0.5] and not ms.quantiles[3]
    assert ptrs[ms.quantiles[0]].dtype == np.float64 and not any(ms.quantile) and not ms.count
    # the three-argument call still works: the limit is the capacity; a field outside `names` gets no list
    ms, keep = N.Context.member_stats_struct(spec, ('ZH',), 1)
    assert ms.quantile_capacity == 128 and list(ms.n_quantiles) == [3] + [0] * 9
    # a plain spec: no quantile terms at all
    ms, keep = N.Context.member_stats_struct(ES.EnsembleStats(), ('ZH',), 3)
    assert ms.quantile_capacity == 0 and ms.quantile_method == 0 and not any(ms.n_quantiles) and not any(ms.quantiles)
    ms, keep = N.Context.member_stats_struct(ES.EnsembleStats(), ('ZH',), 3, capacity=5)
    assert ms.quantile_capacity == 0


def test_the_rule_module_imports_only_numpy():
    tree = ast.parse(open(ES.__file__).read())
    mods = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            mods.append(node.module or '')
    assert mods == ['numpy'], mods
    assert issubclass(ES.EnsembleQuantiles, ES.EnsembleStats)
