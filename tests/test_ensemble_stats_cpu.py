"""Ensemble statistics without a GPU: the rule of ensemble_stats (fold / finish / reduce) against NumPy's float64 nan-aware
reductions and against a plain-Python loop written here from the rule's text, chunk invariance, the edge cases, the refusals
of EnsembleStats, and the layout of cpol_member_stats / cpol_outputs against the header."""
import ast
import ctypes
import inspect
import math
import os
import subprocess
import warnings

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import ensemble_stats as ES
from cosmo_pol_amd import superob as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def members(M, n_cells=1000, seed=0, nan=0.2, dtype=np.float32):
    rng = np.random.default_rng(seed + M)
    x = rng.uniform(1.0, 2.0, (M, n_cells)).astype(dtype)
    x[rng.random(x.shape) < nan] = np.nan
    return x


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def assert_same_stats(a, b, tag=''):
    assert set(a) == set(b), tag
    assert a['n_members'] == b['n_members'], tag
    for kind in a:
        if kind == 'n_members':
            continue
        assert set(a[kind]) == set(b[kind]), (tag, kind)
        for k in a[kind]:
            assert same_bits(a[kind][k], b[kind][k]), (tag, kind, k)


def loop_stats(x, thr, need, T):
    """The rule, cell by cell and member by member, in Python floats (IEEE float64) and NumPy scalars of the field's type."""
    out = {k: [] for k in ('mean', 'spread', 'min', 'max', 'count', 'exceed')}
    thr = [T(t) for t in thr]
    for c in range(x.shape[1]):
        n, mean, M2, lo, hi, k = 0, 0.0, 0.0, T(np.inf), T(-np.inf), [0] * len(thr)
        for v in x[:, c]:
            if v == v:
                n += 1
                d = float(v) - mean
                with np.errstate(all='ignore'):
                    mean = float(np.float64(mean) + np.float64(d) / np.float64(n))
                    M2 = float(np.float64(M2) + np.float64(d) * (np.float64(v) - np.float64(mean)))
                if v < lo:
                    lo = v
                if v > hi:
                    hi = v
                for t, th in enumerate(thr):
                    k[t] += int(v > th)
        out['mean'].append(T(mean) if n >= need else T(np.nan))
        with np.errstate(all='ignore'):
            out['spread'].append(T(np.sqrt(np.float64(M2) / np.float64(n - 1))) if n >= max(need, 2) else T(np.nan))
        out['min'].append(lo if n >= need else T(np.nan))
        out['max'].append(hi if n >= need else T(np.nan))
        out['count'].append(n)
        out['exceed'].append(k)
    return out


@pytest.mark.parametrize('M', [2, 3, 21, 64, 200])
def test_rule_against_numpy_float64(M):
    """Measured here, uniform [1, 2) float32 data, 1000 cells, 20 % NaN, M in {2, 3, 21, 64, 200}: the running float64 mean and
    sqrt(M2 / (n - 1)) deviate from np.nanmean / np.nanstd(ddof=1) by at most 9.0e-16 / 2.2e-15 relative (both worst at M = 200;
    mean / spread: M = 2: 0 / 0, 3: 0 / 9.7e-16, 21: 4.0e-16 / 6.3e-16, 64: 6.1e-16 / 9.8e-16); the bound is 1e-13.  Extremes and counts are exact, and the outputs are those float64 values rounded once."""
    x = members(M)
    thr = [1.25, 1.5, float(np.float32(1.75))]
    spec = ES.EnsembleStats(extremes=True, exceed={'ZH': thr}, fields=['ZH'])
    st = ES.fold(ES.begin(spec, ['ZH'], x.shape[1:]), {'ZH': x})
    s = st['fields']['ZH']
    x64 = x.astype(np.float64)
    n = np.sum(~np.isnan(x), axis=0)
    assert np.array_equal(s['n'], n) and s['n'].dtype == np.uint16
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # (all-NaN cells, one-member cells: NaN is what we want there)
        ref_mean, ref_sd = np.nanmean(x64, axis=0), np.nanstd(x64, axis=0, ddof=1)
        ref_lo, ref_hi = np.nanmin(x64, axis=0), np.nanmax(x64, axis=0)
        sd = np.sqrt(s['M2'] / (n - 1.0))
    ok = n >= 1
    e_mean = np.max(np.abs(s['mean'][ok] - ref_mean[ok]) / np.abs(ref_mean[ok]))
    ok2 = n >= 2
    e_sd = np.max(np.abs(sd[ok2] - ref_sd[ok2]) / ref_sd[ok2])
    print('M = %d: mean %.3g, spread %.3g (relative, against float64 NumPy)' % (M, e_mean, e_sd))
    assert e_mean <= 1e-13 and e_sd <= 1e-13
    res = ES.finish(st, spec)
    assert same_bits(res['mean']['ZH'], np.where(ok, s['mean'], np.nan).astype(np.float32))
    assert same_bits(res['spread']['ZH'], np.where(ok2, sd, np.nan).astype(np.float32))
    assert same_bits(res['min']['ZH'], np.where(ok, ref_lo, np.nan).astype(np.float32))
    assert same_bits(res['max']['ZH'], np.where(ok, ref_hi, np.nan).astype(np.float32))
    assert np.array_equal(res['count']['ZH'], n)
    for t, th in enumerate(thr):
        assert np.array_equal(res['exceed']['ZH'][t], np.sum(x > np.float32(th), axis=0)), th
    assert res['n_members'] == M and res['exceed']['ZH'].dtype == np.uint16
    assert_same_stats(res, ES.reduce({'ZH': x, 'mask': None}, spec))


@pytest.mark.parametrize('name, T', [('KDP', np.float32), ('RVEL', np.float64)])
def test_rule_is_the_python_loop(name, T):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((7, 40)) * 10.0 ** rng.integers(-4, 5, (7, 40))).astype(T)
    x[rng.random(x.shape) < 0.3] = np.nan
    x[:, 0] = np.nan
    x[1:, 1] = np.nan
    thr = [0.0, float(x[2, 5]), -3.0]
    for need in (1, 3):
        spec = ES.EnsembleStats(extremes=True, exceed={name: thr}, fields=[name], min_members=need)
        got = ES.reduce({name: x}, spec)
        want = loop_stats(x, thr, need, T)
        for kind in ('mean', 'spread', 'min', 'max'):
            assert same_bits(got[kind][name], np.array(want[kind], dtype=T)), (kind, need)
        assert np.array_equal(got['count'][name], want['count'])
        assert np.array_equal(got['exceed'][name], np.array(want['exceed']).T)


@pytest.mark.parametrize('M', [2, 5, 21, 200])
def test_chunk_invariance_is_bitwise(M):
    rows = {'ZH': members(M, 300), 'RVEL': members(M, 300, seed=9, dtype=np.float64) * 7.0 - 10.0}
    spec = ES.EnsembleStats(extremes=True, exceed={'ZH': [1.5], 'RVEL': [0.0, 1.0]})
    whole = ES.reduce(rows, spec)
    cuts = [[1] * M, [M - 1, 1], [1, M - 1], [(M + 1) // 2, M // 2], [0, M, 0]]
    for cut in cuts:
        st = ES.begin(spec, ['ZH', 'RVEL'], (300,))
        at = 0
        for n in cut:
            ES.fold(st, {k: v[at:at + n] for k, v in rows.items()})
            at += n
        assert at == M
        assert_same_stats(ES.finish(st, spec), whole, cut)


def test_edge_cases():
    nan, inf = np.nan, np.inf
    f = np.float32
    x = np.array([[nan, 1.0, nan, 2.5, 2.0, 0.0, -0.0, inf, -inf, 1.0],
                  [nan, nan, nan, 2.5, 3.0, -0.0, 0.0, 1.0, -inf, nan],
                  [nan, nan, 4.0, 2.5, 2.0, 0.0, -0.0, 2.0, 1.0, 3.0]], dtype=f)
    spec = ES.EnsembleStats(extremes=True, exceed={'ZH': [2.0, 2.5]}, min_members=2)
    r = ES.reduce({'ZH': x}, spec)
    assert list(r['count']['ZH']) == [0, 1, 1, 3, 3, 3, 3, 3, 3, 2]
    # n < need: everything but the counts is NaN; all NaN: n = 0
    for kind in ('mean', 'spread', 'min', 'max'):
        assert np.isnan(r[kind]['ZH'][:3]).all(), kind
    # n = 1 with need = 1: mean, min and max come, the spread is NaN
    r1 = ES.reduce({'ZH': x}, ES.EnsembleStats(extremes=True))
    assert r1['mean']['ZH'][1] == 1.0 and r1['min']['ZH'][2] == 4.0 and r1['max']['ZH'][2] == 4.0
    assert np.isnan(r1['spread']['ZH'][:3]).all() and np.isnan(r1['mean']['ZH'][0])
    # equal values: the spread is exactly 0
    assert r['spread']['ZH'][3] == 0.0 and not np.signbit(r['spread']['ZH'][3]) and r['mean']['ZH'][3] == f(2.5)
    # a threshold equal to a value does not count it (strict >)
    assert list(r['exceed']['ZH'][:, 3]) == [3, 0] and list(r['exceed']['ZH'][:, 4]) == [1, 1]
    # -0.0 against +0.0: neither is smaller, the first met stays
    assert not np.signbit(r['min']['ZH'][5]) and not np.signbit(r['max']['ZH'][5])
    assert np.signbit(r['min']['ZH'][6]) and np.signbit(r['max']['ZH'][6])
    # infinite members: they count, the extremes carry them, mean and spread follow IEEE
    assert r['max']['ZH'][7] == inf and r['min']['ZH'][7] == 1.0 and r['exceed']['ZH'][0, 7] == 1
    assert np.isnan(r['mean']['ZH'][7]) and np.isnan(r['spread']['ZH'][7])        # inf, then inf - inf
    assert r['min']['ZH'][8] == -inf and r['max']['ZH'][8] == 1.0
    assert r['mean']['ZH'][9] == 2.0 and same_bits(r['spread']['ZH'][9:], np.array([math.sqrt(2.0)], dtype=f))
    p = ES.probability(r, 'ZH')
    assert p.shape == (2, 10) and p[0, 3] == 1.0 and p[0, 9] == 1.0 / 3.0
    pv = ES.probability(r, 'ZH', of='valid')
    assert pv[0, 9] == 0.5 and np.isnan(pv[0, 0])
    assert ES.dbz(35.0) == 10.0 ** 3.5 and np.allclose(ES.dbz([0.0, 10.0]), [1.0, 10.0])
    # the thresholds are compared in the field's type: a double between two float32 values rounds once
    thr = 1.0 + 2.0 ** -30
    r = ES.reduce({'ZH': np.array([[1.0]], dtype=f), 'RVEL': np.array([[1.0 + 2.0 ** -29]])},
                  ES.EnsembleStats(exceed={'ZH': [np.nextafter(f(1.0), f(0.0)).item() + 2.0 ** -30], 'RVEL': [thr]}))
    assert r['exceed']['ZH'][0, 0] == 1 and r['exceed']['RVEL'][0, 0] == 1


def test_refusals():
    for kw in (dict(min_members=0), dict(min_members=65536), dict(min_members=1.5), dict(fields=[]), dict(fields=['ZH', 'ZH']),
               dict(fields=['mask']), dict(exceed={'ZH': [np.nan]}), dict(exceed={'ZH': list(range(9))}), dict(exceed={'ZH': []}),
               dict(exceed={'DSPECTRUM': [1.0]}), dict(exceed={'ZV': [1.0]}, fields=['ZH']), dict(exceed={'ZH': [[1.0]]})):
        with pytest.raises(ValueError):
            ES.EnsembleStats(**kw)
    spec = ES.EnsembleStats(fields=['ZH', 'RVEL'])
    assert spec.fields == ('ZH', 'RVEL') and ES.EnsembleStats(fields=['RVEL', 'ZH']).fields == ('ZH', 'RVEL')
    with pytest.raises(ValueError):                         # RVEL without Doppler
        spec.resolve(['ZH', 'ZV'])
    with pytest.raises(ValueError):
        ES.EnsembleStats(exceed={'RVEL': [0.0]}).resolve(['ZH'])
    assert ES.EnsembleStats().resolve(['ZV', 'ZH', 'mask']) == ('ZH', 'ZV')
    assert ES.EnsembleStats(exceed={'ZH': 3.0}).exceed['ZH'].shape == (1,)
    with pytest.raises(ValueError):
        ES.reduce({'ZH': np.zeros((2, 3))}, ES.EnsembleStats())             # float64 where the field is float32
    with pytest.raises(ValueError):
        ES.probability({'exceed': {}, 'n_members': 1}, 'ZH', of='all')
    assert ES.FIELDS == SO.FIELDS == tuple(N.MEMBER_STATS_FIELDS)
    only = ES.reduce({'ZH': members(3, 10)}, ES.EnsembleStats(mean=False, spread=False))
    assert set(only) == {'count', 'exceed', 'n_members'} and only['exceed'] == {}


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / 'layout.c'
    names = ['phase', 'min_members', 'fields', 'n_thresholds', 'thresholds', 'mean', 'spread', 'min', 'max', 'count', 'exceed']
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "cosmo_pol_amd.h"\nint main(void) {\n'
                   'cpol_outputs o; memset(&o, 0, sizeof o);\n'
                   'printf("%zu %zu %zu %zu %d\\n", sizeof(cpol_member_stats), sizeof(cpol_outputs), offsetof(cpol_outputs, member_stats),\n'
                   '       offsetof(cpol_outputs, superob), o.member_stats == NULL);\n'
                   + ''.join('printf("%%zu\\n", offsetof(cpol_member_stats, %s));\n' % n for n in names)
                   + 'printf("%zu %zu %d %d\\n", sizeof(((cpol_member_stats *)0)->mean), sizeof(((cpol_member_stats *)0)->n_thresholds),\n'
                   '       CPOL_MEMBER_STATS_FIELDS, CPOL_MEMBER_STATS_MAX_THRESHOLDS);\n'
                   'return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    M = N.MemberStats
    assert got == ([ctypes.sizeof(M), ctypes.sizeof(N.Outputs), N.Outputs.member_stats.offset, N.Outputs.superob.offset, 1]
                   + [getattr(M, n).offset for n in names]
                   + [ctypes.sizeof(ctypes.c_void_p) * 10, 40, len(ES.FIELDS), ES.MAX_THRESHOLDS])
    # superob still last, the new member directly before it, and off in a zero-initialised struct
    assert [n for n, _ in N.Outputs._fields_[-2:]] == ['member_stats', 'superob']
    assert N.Outputs.superob.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(N.Outputs)
    assert N.Outputs.member_stats.offset + ctypes.sizeof(ctypes.c_void_p) == N.Outputs.superob.offset
    assert not N.Outputs().member_stats and not N.Outputs().superob
    assert [n for n, _ in N.Outputs._fields_[:-2]] == N.OUTPUT_FIELDS


def test_member_stats_struct_of_a_spec():
    spec = ES.EnsembleStats(exceed={'ZH': [ES.dbz(35.0), 1.0], 'RVEL': [0.0]}, min_members=2)
    ms, keep = N.Context.member_stats_struct(spec, ('ZH', 'KDP', 'RVEL'), 3)
    assert ms.phase == 3 and ms.min_members == 2 and ms.fields == (1 << 0) | (1 << 3) | (1 << 9)
    assert list(ms.n_thresholds) == [2, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert ms.thresholds[0] == keep[0].ctypes.data and ms.thresholds[9] == keep[1].ctypes.data and not ms.thresholds[3]
    assert not ms.count and not any(ms.mean) and not any(ms.exceed)


def test_the_new_methods_exist_and_the_pinned_signatures_stay():
    from cosmo_pol_amd import RadarOperator as R
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(R.simulate_rays_ensemble_stats) == ['self', 'azimuths', 'elevations', 'stats', 'members', 'keep_members', 'form',
                                                   'lane', 'pinned', 'device_outputs', 'apply_sensitivity']
    assert sig(R.get_PPI_ensemble_stats) == ['self', 'elevations', 'stats', 'azimuths', 'az_step', 'az_start', 'az_stop', 'members']
    assert sig(R.get_RHI_ensemble_stats) == ['self', 'azimuths', 'stats', 'elevations', 'elev_step', 'elev_start', 'elev_stop',
                                             'members']
    assert sig(ES.EnsembleStats.__init__) == ['self', 'mean', 'spread', 'extremes', 'exceed', 'fields', 'min_members']
    assert sig(ES.fold) == ['state', 'rows'] and sig(ES.finish)[:2] == ['state', 'spec'] and sig(ES.reduce) == ['fields', 'spec']
    assert sig(ES.probability) == ['stats', 'field', 'of']
    assert callable(N.Context.member_stats_fields)
    # the signatures tests/test_timed_cpu.py pins
    assert sig(R.simulate_rays_at) == ['self', 'azimuths', 'elevations', 'times', 'on_device', 'device_outputs',
                                       'apply_sensitivity', 'lane', 'pinned']
    assert sig(R.load_model_series) == ['self', 'states', 'times', 'zlevels', 'proj_info', 'resolution', 'cfilename']
    assert sig(R.get_PPI_at) == ['self', 'elevations', 'times', 'azimuths', 'az_step', 'az_start', 'az_stop']
    assert sig(R.simulate_rays) == ['self', 'azimuths', 'elevations', 'on_device', 'device_outputs', 'apply_sensitivity', 'paths',
                                    'lane', 'pinned']
    assert sig(R.simulate_rays_ensemble) == ['self', 'azimuths', 'elevations', 'members', 'on_device', 'device_outputs',
                                             'apply_sensitivity', 'lane', 'form', 'pinned', 'superob', 'keep_gates',
                                             'rays_per_block']


def test_the_rule_module_imports_nothing_of_the_oracle():
    tree = ast.parse(open(ES.__file__).read())
    mods = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            mods.append(node.module or '')
    assert mods == ['numpy'], mods
    assert 'oracle' not in open(ES.__file__).read()
