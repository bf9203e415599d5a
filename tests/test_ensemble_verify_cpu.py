"""Ensemble verification without a GPU: the rule of ensemble_verify (`verify`, `reduce`) -- the ranks against a direct count, the
CRPS against the textbook double sum evaluated in np.longdouble --, its edge cases and invariances, the refusals of the spec, the
layout of cpol_member_verify / cpol_outputs against the header, and the host helpers on hand-made cases.

The CRPS bound.  The rule forms the score in float64 and rounds it ONCE to the field's type; the bound 8 n 2^-53 (max|x| + |y|) is
the error of the two float64 sums of n terms (each at most about n 2^-53 relative; the factor 8 is the margin), so it is asserted
on the float64 score before that rounding (`unrounded`), for float32 and float64 members alike -- a float32 result is in addition
asserted to be exactly that float64 score rounded to float32."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import ensemble_stats as ES
from cosmo_pol_amd import ensemble_verify as EV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 2, 3, 5, 21, 64, 127, 128]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def same_verify(a, b):
    return set(a) == set(b) == set(EV.OUTPUTS) and all(same_bits(a[k], b[k]) for k in EV.OUTPUTS)


def textbook(x, y, fair):
    """(1/n) sum |x_i - y| - (1 / 2D) sum_i sum_j |x_i - x_j| in np.longdouble, one cell"""
    L = np.longdouble
    x = np.asarray(x, dtype=L)
    n = len(x)
    D = n * (n - 1) if fair else n * n
    return np.abs(x - L(y)).sum() / L(n) - np.abs(x[:, None] - x[None, :]).sum() / L(2 * D)


@pytest.mark.parametrize('T', [np.float32, np.float64])
@pytest.mark.parametrize('fair', [False, True])
def test_the_rule_on_finite_random_values(T, fair):
    rng = np.random.default_rng(11 + fair + 2 * (T is np.float64))
    worst = 0.0
    for n in NS:
        cells = 150
        x = (rng.standard_normal((n, cells)) * 10.0 ** rng.integers(-3, 4, (1, cells))).astype(T)
        y = (x[rng.integers(0, n, cells), np.arange(cells)].astype(np.float64) + rng.standard_normal(cells) * np.abs(x).max(axis=0)).astype(T)
        y[::10] = x[0, ::10]                                # (an observation that is a member's own value)
        got = EV.verify(x, y, need=1, fair=fair)
        raw = EV.unrounded(x, y, fair)
        assert got['below'].dtype == got['equal'].dtype == np.uint16 and got['crps'].dtype == T
        # the ranks: a direct count (finite values, no zeros of either sign among them: < and == are the rule's order)
        assert np.array_equal(got['below'], (x < y[None]).sum(axis=0)) and np.array_equal(got['equal'], (x == y[None]).sum(axis=0))
        assert (got['equal'][::10] >= 1).all() and (raw['n'] == n).all()
        if fair and n < 2:
            assert np.isnan(got['crps']).all()
            continue
        assert same_bits(got['crps'], raw['r'].astype(T))    # rounded once
        for c in range(cells):
            want = textbook(x[:, c], y[c], fair)
            bound = 8.0 * n * 2.0 ** -53 * (float(np.abs(x[:, c]).max()) + abs(float(y[c])))
            err = float(abs(np.longdouble(raw['r'][c]) - (want if want > 0 else np.longdouble(0))))
            assert err <= bound, (n, c, err, bound)
            worst = max(worst, err / bound)
    print('worst error / bound: %.3f' % worst)
    assert worst < 1.0


def test_nan_members_do_not_count():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((21, 300)).astype(np.float32)
    x[rng.random(x.shape) < 0.3] = np.nan
    x[:, 0] = np.nan
    y = rng.standard_normal(300).astype(np.float32)
    got = EV.verify(x, y)
    assert got['below'][0] == 0 and got['equal'][0] == 0 and np.isnan(got['crps'][0])
    for c in range(1, 300):
        col = x[:, c][~np.isnan(x[:, c])]
        one = EV.verify(col[:, None], y[c:c + 1])
        assert all(same_bits(one[k][0], got[k][c]) for k in EV.OUTPUTS), c
        assert got['below'][c] == (col < y[c]).sum()


def test_edge_cases():
    nan, inf = np.nan, np.inf
    for T in (np.float32, np.float64):
        a = lambda *v: np.array(v, dtype=T)
        x = np.stack([a(1, 2, 3), a(2, 2, nan), a(3, 2, nan)])           # cells: (1, 2, 3), (2, 2, 2), (3)
        # a NaN observation: ranks 0, crps NaN
        got = EV.verify(x, a(nan, nan, nan))
        assert not got['below'].any() and not got['equal'].any() and np.isnan(got['crps']).all()
        # n < need gates the CRPS, never the ranks; n == 0; fair with n == 1
        got = EV.verify(x, a(2, 2, 2), need=2)
        assert got['below'].tolist() == [1, 0, 0] and got['equal'].tolist() == [1, 3, 0] and np.isnan(got['crps'][2])
        assert got['crps'][1] == 0 and got['crps'].dtype == T
        assert np.isnan(EV.verify(np.full((2, 1), nan, T), a(1.0))['crps'][0])
        assert np.isnan(EV.verify(np.zeros((0, 1), T), a(1.0))['crps'][0]) and EV.verify(np.zeros((0, 1), T), a(1.0))['below'][0] == 0
        one = EV.verify(x, a(2, 2, 2), fair=True)
        assert np.isnan(one['crps'][2]) and one['equal'][2] == 0 and one['below'][2] == 0 and one['crps'][1] == 0
        assert EV.verify(x, a(2, 2, 2))['crps'][2] == 1.0                # |3 - 2|, no pair term
        # (1, 2, 3) against 2: A = 2, B = -2 * 1 + 0 * 2 + 2 * 3 = 4, D = 9 (fair: 6) -- the pair sum 1 + 2 + 1, twice, is 2 B
        assert got['crps'][0] == T(2.0 / 3.0 - 4.0 / 9.0) and one['crps'][0] == T(2.0 / 3.0 - 4.0 / 6.0) == 0
        # all members equal to the observation: crps == +0.0, fair or not
        for fair in (False, True):
            z = EV.verify(np.full((5, 4), 1.25, T), np.full(4, 1.25, T), fair=fair)
            assert same_bits(z['crps'], np.zeros(4, T)) and (z['equal'] == 5).all() and not z['below'].any()
        # ties
        t = np.stack([a(1.0), a(2.0), a(2.0), a(2.0), a(5.0)])
        assert [int(EV.verify(t, a(v))[k][0]) for v in (0.5, 2.0, 3.0, 5.0, 6.0) for k in ('below', 'equal')] == [0, 0, 1, 3, 4, 0, 4, 1, 5, 0]
        # +-0.0: -0.0 comes before +0.0
        zz = np.stack([a(-0.0), a(0.0), a(0.0)])
        assert [int(EV.verify(zz, a(v))[k][0]) for v in (-0.0, 0.0) for k in ('below', 'equal')] == [0, 1, 1, 2]
        assert same_bits(EV.verify(zz, a(-0.0))['crps'], a(0.0))
        # +-inf: ordered like any value; the CRPS is what IEEE gives
        ii = np.stack([a(-inf), a(1.0), a(inf)])
        assert [int(EV.verify(ii, a(v))[k][0]) for v in (-inf, 0.0, inf) for k in ('below', 'equal')] == [0, 1, 1, 0, 2, 1]
        assert np.isnan(EV.verify(ii, a(0.0))['crps'][0])                # (B: -2 * -inf + 0 + 2 * inf = inf; inf - inf)
        assert np.isnan(EV.verify(np.stack([a(1.0), a(inf)]), a(0.0))['crps'][0])       # inf / 2 - inf / 4
        assert EV.verify(np.stack([a(1.0), a(2.0)]), a(inf))['crps'][0] == inf
    with pytest.raises(ValueError):
        EV.verify(np.zeros((2, 3), np.float32), np.zeros(3, np.float64))
    with pytest.raises(ValueError):
        EV.verify(np.zeros((2, 3), np.float32), np.zeros(4, np.float32))
    with pytest.raises(ValueError, match='128'):
        EV.verify(np.zeros((129, 3), np.float32), np.zeros(3, np.float32))


def rows_and_obs(M=21, cells=200, seed=5):
    rng = np.random.default_rng(seed)
    rows = {}
    for k in ('ZH', 'KDP', 'RVEL'):
        x = rng.standard_normal((M, cells)).astype(ES.dtype_of(k))
        x[rng.random(x.shape) < 0.2] = np.nan
        rows[k] = x
    obs = {k: (v[3] * ES.dtype_of(k)(1.3)) for k, v in rows.items()}
    for v, x in zip(obs.values(), rows.values()):
        v[::11] = x[M - 1, ::11]
    return rows, obs


def test_invariances():
    rows, obs = rows_and_obs()
    spec = EV.EnsembleVerification(verify=('ZH', 'RVEL'), quantiles={'KDP': [0.5]}, fields=['ZH', 'KDP', 'RVEL'], min_members=2)
    want = EV.reduce(rows, obs, spec)
    assert set(want) == {'mean', 'spread', 'count', 'exceed', 'quantile', 'verify', 'n_members'}
    assert set(want['verify']) == set(EV.OUTPUTS) and all(set(v) == {'ZH', 'RVEL'} for v in want['verify'].values())
    assert want['verify']['crps']['RVEL'].dtype == np.float64 and want['verify']['crps']['ZH'].dtype == np.float32
    own = ~np.isnan(obs['ZH'][::11])                         # (an observation that is a member's own value ties with it)
    assert np.isfinite(want['verify']['crps']['ZH']).any() and own.any() and (want['verify']['equal']['ZH'][::11][own] >= 1).all()
    # the statistics beside it are those of the plain reduce
    plain = ES.reduce(rows, spec)
    for kind in ('mean', 'spread', 'count', 'quantile'):
        assert all(same_bits(want[kind][k], plain[kind][k]) for k in plain[kind])
    # permuting the members: the same bits of the three outputs
    p = np.random.default_rng(1).permutation(21)
    got = EV.reduce({k: v[p] for k, v in rows.items()}, obs, spec)
    assert all(same_verify({o: got['verify'][o][k] for o in EV.OUTPUTS}, {o: want['verify'][o][k] for o in EV.OUTPUTS}) for k in ('ZH', 'RVEL'))
    # the pass cut through begin / fold / finish
    for cut in ([21], [1] * 21, [20, 1], [7, 0, 14]):
        st = ES.begin(spec, ['ZH', 'KDP', 'RVEL'], (200,))
        at = 0
        for n in cut:
            st = ES.fold(st, {k: v[at:at + n] for k, v in rows.items()})
            at += n
        got = EV.finish(st, obs)
        for kind, w in want.items():
            if kind == 'n_members':
                continue
            for k, v in (w.items() if kind != 'verify' else [((o, f), a) for o, d in w.items() for f, a in d.items()]):
                g = got[kind][k] if kind != 'verify' else got['verify'][k[0]][k[1]]
                assert same_bits(g, v), (cut, kind, k)
    # verify() == the reduce, field by field; need and fair arrive
    v = EV.verify(rows['ZH'], obs['ZH'], need=2)
    assert same_verify(v, {o: want['verify'][o]['ZH'] for o in EV.OUTPUTS})
    fair = EV.reduce(rows, obs, EV.EnsembleVerification(verify=['ZH'], fair=True, fields=['ZH']))
    assert 'quantile' not in fair and same_bits(fair['verify']['crps']['ZH'], EV.verify(rows['ZH'], obs['ZH'], fair=True)['crps'])
    assert not same_bits(fair['verify']['crps']['ZH'], want['verify']['crps']['ZH'])


def test_refusals_and_the_spec():
    V = EV.EnsembleVerification
    for kw in (dict(verify=['DSPECTRUM']), dict(verify=['ZH', 'ZH']), dict(verify=[]), dict(verify=['ZV'], fields=['ZH']),
               dict(fair=1), dict(fair=None), dict(fair='yes'), dict(quantiles={'ZH': [1.5]}), dict(quantiles={'ZV': 0.5}, fields=['ZH']),
               dict(min_members=0), dict(method='median')):
        with pytest.raises(ValueError):
            V(**kw)
    spec = V()
    assert isinstance(spec, ES.EnsembleQuantiles) and spec.verify == ('ZH',) and spec.fair is False and spec.quantiles == {}
    spec = V(verify=('RVEL', 'ZH'), fair=True, quantiles={'ZH': 0.5}, method='lower', extremes=True, min_members=3)
    assert spec.verify == ('ZH', 'RVEL') and spec.fair is True and spec.method == 'lower' and spec.extremes and spec.min_members == 3
    assert V(verify='KDP').verify == ('KDP',)
    with pytest.raises(ValueError):                         # RVEL without Doppler
        spec.resolve(['ZH', 'ZV'])
    assert spec.resolve(['ZH', 'RVEL', 'mask']) == ('ZH', 'RVEL')
    assert spec.key != V(verify=('RVEL', 'ZH'), fair=False, quantiles={'ZH': 0.5}, method='lower', extremes=True, min_members=3).key
    assert spec.key != V(verify=('ZH',), fair=True, quantiles={'ZH': 0.5}, method='lower', extremes=True, min_members=3).key
    assert repr(spec).startswith('EnsembleVerification(') and 'RVEL' in repr(spec)
    # the observations of a reduce: a missing field, a wrong dtype, a wrong shape
    rows, obs = rows_and_obs(5, 20)
    spec = V(verify=('ZH', 'RVEL'), fields=['ZH', 'RVEL'])
    for bad in ({'ZH': obs['ZH']}, dict(obs, RVEL=obs['RVEL'].astype(np.float32)), dict(obs, ZH=obs['ZH'][:-1]), [obs['ZH']], None):
        with pytest.raises(ValueError):
            EV.reduce(rows, bad, spec)
    # more than 128 members
    with pytest.raises(ValueError, match='128'):
        EV.reduce({'ZH': np.ones((129, 3), np.float32)}, {'ZH': np.ones(3, np.float32)}, V())
    # a plain spec keeps no members; a verified field without quantiles does
    st = ES.begin(V(verify=['ZH'], quantiles={'KDP': 0.5}), ['ZH', 'ZV', 'KDP'], (3,))
    assert 'x' in st['fields']['ZH'] and 'x' in st['fields']['KDP'] and 'x' not in st['fields']['ZV']
    assert EV.MAX_MEMBERS == 128 and EV.OUTPUTS == ('below', 'equal', 'crps')


def test_struct_layout_matches_header(tmp_path):
    names = ['fields', 'fair', 'obs', 'below', 'equal', 'crps']
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "cosmo_pol_amd.h"\nint main(void) {\n'
                   'cpol_outputs o; memset(&o, 0, sizeof o);\n'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(cpol_member_verify), sizeof(cpol_outputs), offsetof(cpol_outputs, DSPECTRUM),\n'
                   '       offsetof(cpol_outputs, member_verify), offsetof(cpol_outputs, mask_sum8), o.member_verify == NULL);\n'
                   + ''.join('printf("%%zu %%zu\\n", offsetof(cpol_member_verify, %s), sizeof(((cpol_member_verify *)0)->%s));\n' % (n, n)
                             for n in names)
                   + ''.join('printf("%%zu\\n", offsetof(cpol_outputs, %s));\n' % n for n, _ in N.Outputs._fields_)
                   + 'return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    M, O = N.MemberVerify, N.Outputs
    ptr = ctypes.sizeof(ctypes.c_void_p)
    want = [ctypes.sizeof(M), ctypes.sizeof(O), O.DSPECTRUM.offset, O.member_verify.offset, O.mask_sum8.offset, 1]
    for n in names:
        want += [getattr(M, n).offset, getattr(M, n).size]
    want += [getattr(O, n).offset for n, _ in O._fields_]
    assert got == want
    assert [n for n, _ in M._fields_] == names and M.obs.offset == 8 and M.obs.size == M.crps.size == 10 * ptr
    assert M.crps.offset + 10 * ptr == ctypes.sizeof(M)
    # member_verify sits directly before mask_sum8, behind the last array; the last four members are where they were
    assert O.member_verify.offset == O.DSPECTRUM.offset + ptr and O.mask_sum8.offset == O.member_verify.offset + ptr
    assert [n for n, _ in O._fields_[-5:]] == ['member_verify', 'mask_sum8', 'spectrum_moments', 'member_stats', 'superob']
    assert [n for n, _ in O._fields_[:-2]] == N.OUTPUT_FIELDS and N.OUTPUT_FIELDS.index('member_verify') == N.OUTPUT_FIELDS.index('mask_sum8') - 1
    assert O.superob.offset + ptr == ctypes.sizeof(O)
    z = O()
    assert not z.member_verify and not z.member_stats
    zm = M()
    assert zm.fields == 0 and zm.fair == 0 and not any(zm.obs) and not any(zm.crps)
    # no new exported name: the hook is a control name of cpol_debug_read
    assert len(N.EXPORTS) == 37 and not [n for n in N.EXPORTS if 'verify' in n]
    text = open(os.path.join(ROOT, 'cosmo_pol_amd', 'csrc', 'exports.map')).read()
    assert 'verify' not in text


def test_structs_of_a_spec():
    spec = EV.EnsembleVerification(verify=('ZH', 'RVEL'), fair=True, min_members=2)
    mv = N.Context.member_verify_struct(spec)
    assert mv.fields == (1 << 0) | (1 << 9) and mv.fair == 1 and not any(mv.obs) and not any(mv.below)
    # a verified field keeps its members like a field with quantiles: the capacity goes with the statistics struct
    ms, keep = N.Context.member_stats_struct(spec, ('ZH', 'RVEL'), 3, capacity=21)
    assert ms.quantile_capacity == 21 and not any(ms.n_quantiles) and ms.fields == mv.fields
    assert N.Context.member_stats_struct(spec, ('ZH', 'RVEL'), 1)[0].quantile_capacity == 128
    assert N.Context.member_stats_struct(ES.EnsembleStats(), ('ZH',), 3)[0].quantile_capacity == 0


def test_the_entry_points_exist_beside_the_pinned_ones():
    import inspect
    from cosmo_pol_amd import RadarOperator as R
    sig = lambda f: list(inspect.signature(f).parameters)
    # (tests/test_ensemble_stats_cpu.py pins the parameter lists of the statistics calls: the observations enter through calls of their own)
    assert sig(R.simulate_rays_ensemble_verify) == ['self', 'azimuths', 'elevations', 'stats', 'observations', 'members', 'keep_members',
                                                    'form', 'lane', 'pinned', 'device_outputs', 'apply_sensitivity']
    assert sig(R.get_PPI_ensemble_verify) == ['self', 'elevations', 'stats', 'observations', 'azimuths', 'az_step', 'az_start', 'az_stop',
                                              'members']
    assert sig(R.get_RHI_ensemble_verify) == ['self', 'azimuths', 'stats', 'observations', 'elevations', 'elev_step', 'elev_start',
                                              'elev_stop', 'members']
    assert sig(EV.verify) == ['x', 'y', 'need', 'fair'] and sig(EV.reduce) == ['fields', 'observations', 'spec']
    assert sig(EV.rank_histogram)[:5] == ['below', 'equal', 'count', 'n_members', 'ties'] and sig(EV.brier)[:3] == ['stats', 'observed', 'field']
    assert sig(N.Context.member_verify_fields)[:5] == ['self', 'fields', 'observations', 'spec', 'phase']
    assert 'observations' not in sig(R.simulate_rays_ensemble_stats)


def test_rank_histogram():
    below = np.array([0, 3, 1, 1, 2, 0, 0])
    equal = np.array([0, 0, 0, 1, 1, 3, 0])
    count = np.array([3, 3, 3, 3, 3, 3, 2])                 # (the last gate: a member did not count -- left out)
    h = EV.rank_histogram(below, equal, count, 3)
    assert h.dtype == np.float64 and h.shape == (4,)
    # gate 3 spreads over bins 1, 2; gate 4 over bins 2, 3; gate 5 over all four
    assert np.allclose(h, [1 + 0.25, 1 + 0.5 + 0.25, 0.5 + 0.5 + 0.25, 1 + 0.5 + 0.25]) and abs(h.sum() - 6.0) < 1e-12
    assert EV.rank_histogram(below, equal, count, 3, ties='low').tolist() == [2, 2, 1, 1]
    assert EV.rank_histogram(below, equal, count, 3, ties='high').tolist() == [1, 1, 1, 3]
    # gates without an observation are left out
    present = np.array([0, 1, 1, 1, 1, 1, 1], bool)
    assert np.allclose(EV.rank_histogram(below, equal, count, 3, present=present), [0.25, 1.75, 1.25, 1.75])
    assert EV.rank_histogram(below.reshape(7, 1), equal.reshape(7, 1), count.reshape(7, 1), 3).shape == (4,)
    assert not EV.rank_histogram(below, equal, count, 4).any()
    for kw in (dict(ties='mid'), dict(present=present[:3])):
        with pytest.raises(ValueError):
            EV.rank_histogram(below, equal, count, 3, **kw)
    with pytest.raises(ValueError):
        EV.rank_histogram(below + 3, equal, count, 3)
    # a flat histogram from the rule itself: an observation drawn like the members
    rng = np.random.default_rng(0)
    x = rng.standard_normal((9, 20000)).astype(np.float32)
    v = EV.verify(x[1:], x[0])
    h = EV.rank_histogram(v['below'], v['equal'], np.full(20000, 8), 8)
    assert h.sum() == 20000 and np.abs(h / 20000 - 1 / 9).max() < 0.01


def test_brier():
    spec = ES.EnsembleStats(exceed={'ZH': [1.0, 10.0]})
    stats = {'exceed': {'ZH': np.array([[4, 0, 2, 4], [0, 0, 2, 1]], np.uint16)}, 'n_members': 4}
    observed = np.array([2.0, 0.5, 20.0, np.nan], np.float32)
    b = EV.brier(stats, observed, 'ZH', spec)
    # threshold 1: p = 1, 0, 0.5 against 1, 0, 1; threshold 10: p = 0, 0, 0.5 against 0, 0, 1; the NaN gate is left out
    assert b.dtype == np.float64 and np.allclose(b, [0.25 / 3, 0.25 / 3])
    assert np.allclose(EV.brier(stats, observed, 'ZH', [1.0, 30.0]), [0.25 / 3, 0.25 / 3 ])
    assert np.isnan(EV.brier(stats, np.full(4, np.nan, np.float32), 'ZH', spec)).all()
    with pytest.raises(ValueError):
        EV.brier(stats, observed[:3], 'ZH', spec)
    with pytest.raises(ValueError):
        EV.brier(stats, observed, 'ZH', [1.0])
