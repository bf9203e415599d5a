"""Spectrum moments without a GPU: the NumPy statement of the rule (cosmo_pol_amd/spectrum_moments.py) against an independent
formulation (math.fsum) on the committed spectra, closed forms, what counts, the stated order of the sums (a scalar loop written
from the header's text), the operator's new methods beside the pinned signatures, and the ctypes structs against the header."""
import ast
import copy
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

import _cases
from cosmo_pol_amd import _native as N
from cosmo_pol_amd import spectrum_moments as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECTRA = ('radial_d3_turb_motion_fft256', 'radial_d3_turb_masked', 'radial_d3_melt')
ALL = SM.SpectrumMoments(fields=SM.FIELDS)


def fixture_varray(g, name):
    """the fixture's own velocity bins, else those of the operator's constants for the fixture's configuration"""
    if 'varray' in g.files:
        return np.ascontiguousarray(g['varray'], dtype=np.float64)
    from cosmo_pol_amd import config as cfg
    from cosmo_pol_amd import constants
    over = _cases.gen_golden.radial_case_inputs(name[len('radial_'):])[0]
    return np.ascontiguousarray(constants.DerivedConstants(cfg.sanity_check(copy.deepcopy(over))).VARRAY, dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want, what=''):
    """NaN where `want` has NaN, identical bits everywhere else"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), what


def scalar_gate(S, V, min_power=0.0, min_bins=1):
    """One gate by a scalar loop written from the text of include/cosmo_pol_amd.h (np.float64 scalars: IEEE operations, and a
    division by zero gives what IEEE gives)."""
    f = np.float64
    n_v = len(S)
    S, V = [f(x) for x in S], [f(x) for x in V]
    counts = [bool(S[v] == S[v] and S[v] > min_power) for v in range(n_v)]
    n = sum(counts)

    def R(t):
        a = [f(0.0)] * 64
        for lane in range(64):
            v = lane
            while v < n_v:
                if counts[v]:
                    a[lane] = a[lane] + t(v)
                v += 64
        for off in (32, 16, 8, 4, 2, 1):
            a = [a[lane] + a[lane ^ off] for lane in range(64)]
        assert all(x.tobytes() == a[0].tobytes() or (x != x and a[0] != a[0]) for x in a)     # all lanes hold the same value
        return a[0]
    with np.errstate(all='ignore'):
        P = R(lambda v: S[v])
        M = R(lambda v: V[v] * S[v])
        vbar = M / P
        d = lambda v: V[v] - vbar
        C2 = R(lambda v: (d(v) * d(v)) * S[v])
        C3 = R(lambda v: ((d(v) * d(v)) * d(v)) * S[v])
        C4 = R(lambda v: ((d(v) * d(v)) * (d(v) * d(v))) * S[v])
        var = C2 / P
        width = np.sqrt(var)
        out = {'POWER': P, 'VMEAN': vbar, 'WIDTH': width, 'SKEWNESS': (C3 / P) / (var * width), 'KURTOSIS': (C4 / P) / (var * var)}
    idx = [v for v in range(n_v) if counts[v]]
    if idx:
        top = max(S[v] for v in idx)
        out['VPEAK'] = V[min(v for v in idx if S[v] == top)]
        out['VLOW'], out['VHIGH'] = V[idx[0]], V[idx[-1]]
    if n < min_bins or not idx:
        out = {k: f('nan') for k in SM.FIELDS}
    out['count'] = n
    return out


@pytest.mark.parametrize('name', SPECTRA)
def test_rule_against_fsum_on_the_committed_spectra(golden, name):
    """P, M, C2, C3, C4 of every gate within n_v * 2^-52 * sum|term| of the exactly rounded sum of the same terms: the bound of
    ANY summation order of n_v terms (n_v - 1 additions of relative error 2^-53 each, to first order), taken twice."""
    g = golden(name)
    V = fixture_varray(g, name)
    n_v = len(V)
    for key in ('cutll_DSPECTRUM', 'obs_DSPECTRUM'):
        S = np.ascontiguousarray(g[key], dtype=np.float64)
        assert S.shape[1] == n_v
        r = SM.sums(S, V, ALL)
        out = SM.moments(S, V, ALL)
        assert np.array_equal(out['count'], r['n'])
        checked = 0
        for i in range(S.shape[0]):
            c = r['counts'][i]
            assert r['n'][i] == int(c.sum())
            if not c.any():
                assert np.isnan(out['POWER'][i])
                continue
            s, v = S[i][c], V[c]
            d = v - r['vbar'][i]
            d2 = d * d
            for what, terms in (('P', s), ('M', v * s), ('C2', d2 * s), ('C3', (d2 * d) * s), ('C4', (d2 * d2) * s)):
                exact = math.fsum(terms)
                bound = n_v * 2.0 ** -52 * math.fsum(np.abs(terms))
                assert abs(r[what][i] - exact) <= bound, (name, key, i, what, r[what][i], exact, bound)
            checked += 1
        assert checked == int((r['n'] > 0).sum()) and checked > 20, (name, key, checked)     # (not vacuous)
        if key == 'cutll_DSPECTRUM':
            assert np.isnan(S).any() and not np.isnan(S).all()              # (the cut spectra carry censored bins)
        kur = out['KURTOSIS'][r['n'] > 8]
        assert np.all(kur[np.isfinite(kur)] >= 1.0)                         # (kurtosis >= 1 + skewness^2 >= 1)


def test_closed_forms():
    V = np.linspace(-8.0, 8.0, 129)
    # one counting bin: width 0, skewness and kurtosis NaN
    S = np.zeros((1, 129))
    S[0, 40] = 2.5
    r = SM.moments(S, V, ALL)
    assert r['count'][0] == 1 and r['POWER'][0] == 2.5 and r['VMEAN'][0] == V[40] and r['WIDTH'][0] == 0.0
    assert np.isnan(r['SKEWNESS'][0]) and np.isnan(r['KURTOSIS'][0])
    assert r['VPEAK'][0] == r['VLOW'][0] == r['VHIGH'][0] == V[40]
    # two equal bins at +-v: mean 0, width v, skewness 0, kurtosis 1
    S = np.zeros((1, 129))
    S[0, 64 - 24] = S[0, 64 + 24] = 0.75
    assert V[64 - 24] == -3.0 and V[64 + 24] == 3.0
    r = SM.moments(S, V, ALL)
    assert r['count'][0] == 2 and r['POWER'][0] == 1.5 and r['VMEAN'][0] == 0.0 and r['WIDTH'][0] == 3.0
    assert r['SKEWNESS'][0] == 0.0 and r['KURTOSIS'][0] == 1.0
    assert r['VPEAK'][0] == -3.0 and r['VLOW'][0] == -3.0 and r['VHIGH'][0] == 3.0
    # all bins equal: the peak is the first bin
    r = SM.moments(np.full((2, 129), 0.3), V, ALL)
    assert np.all(r['VPEAK'] == V[0]) and np.all(r['VLOW'] == V[0]) and np.all(r['VHIGH'] == V[128]) and np.all(r['count'] == 129)
    # a tie between bin 63 and bin 64 (two lanes, two rounds of the lane loop): the lower index
    S = np.full((1, 129), 0.1)
    S[0, 63] = S[0, 64] = 7.0
    assert SM.moments(S, V, ALL)['VPEAK'][0] == V[63]
    S[0, 63] = np.nextafter(7.0, 0.0)
    assert SM.moments(S, V, ALL)['VPEAK'][0] == V[64]


def test_counting():
    V = np.linspace(-4.0, 4.0, 70)
    rng = np.random.default_rng(3)
    S = rng.random((4, 70)) + 0.5
    S[:, 0] = np.nan
    S[:, 5] = 0.0
    S[:, 6] = -0.0
    S[:, 7] = -1.0
    S[:, 69] = np.nan
    S[1, :] = np.nan                                                        # a gate without a counting bin
    S[2, 10:] = 0.0                                                         # a gate with 5 (bins 1-4, 8, 9 -> 6) counting bins
    r = SM.moments(S, V, ALL)
    assert list(r['count']) == [65, 0, 6, 65]
    assert all(np.isnan(r[k][1]) for k in SM.FIELDS)
    assert r['VLOW'][0] == V[1] and r['VHIGH'][0] == V[68] and r['VHIGH'][2] == V[9]
    keep = np.ones(70, bool)
    keep[[0, 5, 6, 7, 69]] = False
    assert abs(r['POWER'][0] - math.fsum(S[0][keep])) <= 70 * 2.0 ** -52 * math.fsum(S[0][keep])
    # min_power excludes what is not above it (a bin AT min_power does not count)
    S2 = np.array([[0.5, 1.0, 2.0, 1.0, 0.25]])
    V2 = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    r = SM.moments(S2, V2, SM.SpectrumMoments(fields=SM.FIELDS, min_power=0.5))
    assert r['count'][0] == 3 and r['POWER'][0] == 4.0 and r['VMEAN'][0] == 0.0 and r['VLOW'][0] == -1.0 and r['VHIGH'][0] == 1.0
    r = SM.moments(S2, V2, SM.SpectrumMoments(fields=SM.FIELDS, min_power=1.0))
    assert r['count'][0] == 1 and r['POWER'][0] == 2.0 and r['WIDTH'][0] == 0.0
    # min_bins above n: NaN, count kept
    r = SM.moments(S2, V2, SM.SpectrumMoments(fields=SM.FIELDS, min_power=0.5, min_bins=4))
    assert r['count'][0] == 3 and all(np.isnan(r[k][0]) for k in SM.FIELDS)
    r = SM.moments(S2, V2, SM.SpectrumMoments(fields=SM.FIELDS, min_power=0.5, min_bins=3))
    assert r['POWER'][0] == 4.0
    # shapes: [..., n_v] -> [...]
    r = SM.moments(np.ones((2, 3, 5)), V2, SM.SpectrumMoments())
    assert set(r) == {'POWER', 'VMEAN', 'WIDTH', 'count'} and r['WIDTH'].shape == (2, 3) and r['count'].dtype == np.uint16
    with pytest.raises(ValueError):
        SM.moments(np.ones((2, 5), np.float32), V2, SM.SpectrumMoments())
    with pytest.raises(ValueError):
        SM.moments(np.ones((2, 4)), V2, SM.SpectrumMoments())


def test_the_order_is_the_stated_one(golden):
    """Gates recomputed by the scalar loop of the header's text: the same bits.  Reversing the velocity bins and the row
    together changes which lane and which round a bin falls into: again the scalar loop's bits, and sums that differ from the
    forward ones by no more than the bound of the summation."""
    name = 'radial_d3_turb_motion_fft256'
    g = golden(name)
    V = fixture_varray(g, name)
    # (Reversing n_v bins maps lane l to lane (n_v - 1 - l) mod 64, which keeps every residue class mod 2, 4, ... 32 a class: the
    # butterfly adds the same sets.  The bits can change only where a lane holds three or more counting bins, whose order inside
    # the lane reverses.  These spectra fill half of their 257 bins with sums of a few float32 values, exact in any order: the
    # empty bins get a weak random floor and every bin a random factor in [1, 2), so that the order of the additions shows.)
    rng = np.random.default_rng(5)
    S = np.ascontiguousarray(g['obs_DSPECTRUM'][:, 3:], dtype=np.float64)
    S = np.where(S == 0.0, 1e-3 * rng.random(S.shape), S * (1.0 + rng.random(S.shape)))
    S[:, ::11] = np.nan                                                     # (censored bins, as the sensitivity cut leaves them)
    V = np.ascontiguousarray(V[3:])
    gates = [int(i) for i in np.argsort(-(S > 0).sum(1), kind='stable')[:4]]          # (two asked for; four, so that the order shows)
    assert all((S[i] > 0).sum() > 128 for i in gates) and np.isnan(S[gates]).any()       # (a lane with three bins; censored bins)
    differs = False
    for spec in (ALL, SM.SpectrumMoments(fields=SM.FIELDS, min_power=float(np.nanmedian(S[gates[0]])), min_bins=3)):
        fwd = SM.moments(S[gates], V, spec)
        rev = SM.moments(S[gates][:, ::-1], V[::-1], spec)
        for j, i in enumerate(gates):
            for Sg, Vg, got in ((S[i], V, fwd), (S[i][::-1], V[::-1], rev)):
                want = scalar_gate(Sg, Vg, spec.min_power, spec.min_bins)
                assert got['count'][j] == want['count']
                for k in SM.FIELDS:
                    assert_same_bits(got[k][j], want[k], (i, k))
            n_v = len(V)
            c = np.isfinite(S[i]) & (S[i] > spec.min_power)
            assert abs(fwd['POWER'][j] - rev['POWER'][j]) <= 2 * n_v * 2.0 ** -52 * math.fsum(S[i][c])
            assert fwd['VPEAK'][j] == rev['VPEAK'][j] and fwd['VLOW'][j] == rev['VHIGH'][j] and fwd['VHIGH'][j] == rev['VLOW'][j]
            differs = differs or any(bits(fwd[k][j]) != bits(rev[k][j]) for k in ('POWER', 'VMEAN', 'WIDTH', 'SKEWNESS', 'KURTOSIS'))
    assert differs                                                          # (the order matters: the test is not vacuous)


def test_specification_refusals():
    assert SM.FIELDS == tuple(N.SPECTRUM_MOMENTS_FIELDS) and len(SM.FIELDS) == 8
    s = SM.SpectrumMoments()
    assert s.fields == ('POWER', 'VMEAN', 'WIDTH') and s.min_power == 0.0 and s.min_bins == 1 and s.mask == 0b111
    assert SM.SpectrumMoments(fields=('VHIGH', 'POWER')).fields == ('POWER', 'VHIGH')
    assert SM.SpectrumMoments(fields='KURTOSIS').mask == 1 << 4 and ALL.mask == 0xFF
    for kw in (dict(fields=()), dict(fields=('ZH',)), dict(min_bins=0), dict(min_bins=65536), dict(min_bins=1.5),
               dict(min_power=-1e-300), dict(min_power=float('nan')), dict(min_power=float('inf'))):
        with pytest.raises(ValueError):
            SM.SpectrumMoments(**kw)
    assert SM.SpectrumMoments(min_bins=65535, min_power=1e300).min_bins == 65535
    sm = N.Context.spectrum_moments_struct(SM.SpectrumMoments(fields=('WIDTH', 'VLOW'), min_power=0.25, min_bins=7))
    assert (sm.fields, sm.min_bins, sm.min_power) == ((1 << 2) | (1 << 6), 7, 0.25) and not sm.moments and not sm.count


def test_the_new_methods_exist_and_the_pinned_signatures_stay():
    from cosmo_pol_amd import RadarOperator as R
    from cosmo_pol_amd import ensemble_stats as ES
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(R.simulate_rays_moments) == ['self', 'azimuths', 'elevations', 'moments', 'keep_spectrum', 'device_outputs',
                                            'apply_sensitivity', 'paths', 'lane', 'pinned']
    assert sig(R.get_PPI_moments) == ['self', 'elevations', 'moments', 'azimuths', 'az_step', 'az_start', 'az_stop', 'keep_spectrum']
    assert sig(R.get_RHI_moments) == ['self', 'azimuths', 'moments', 'elevations', 'elev_step', 'elev_start', 'elev_stop',
                                      'keep_spectrum']
    assert sig(SM.SpectrumMoments.__init__) == ['self', 'fields', 'min_power', 'min_bins']
    assert sig(SM.moments) == ['spectrum', 'varray', 'spec']
    assert sig(N.Context.spectrum_moments_rows)[:4] == ['self', 'spectrum', 'varray', 'spec']
    d = inspect.signature(R.simulate_rays_moments).parameters
    assert (d['keep_spectrum'].default, d['device_outputs'].default, d['apply_sensitivity'].default, d['paths'].default,
            d['lane'].default, d['pinned'].default) == (False, None, True, None, 0, False)
    # every signature tests/test_ensemble_stats_cpu.py pins
    assert sig(R.simulate_rays_ensemble_stats) == ['self', 'azimuths', 'elevations', 'stats', 'members', 'keep_members', 'form',
                                                   'lane', 'pinned', 'device_outputs', 'apply_sensitivity']
    assert sig(R.get_PPI_ensemble_stats) == ['self', 'elevations', 'stats', 'azimuths', 'az_step', 'az_start', 'az_stop', 'members']
    assert sig(R.get_RHI_ensemble_stats) == ['self', 'azimuths', 'stats', 'elevations', 'elev_step', 'elev_start', 'elev_stop',
                                             'members']
    assert sig(ES.EnsembleStats.__init__) == ['self', 'mean', 'spread', 'extremes', 'exceed', 'fields', 'min_members']
    assert sig(ES.fold) == ['state', 'rows'] and sig(ES.finish)[:2] == ['state', 'spec'] and sig(ES.reduce) == ['fields', 'spec']
    assert sig(ES.probability) == ['stats', 'field', 'of']
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
    text = open(SM.__file__).read()
    mods = []
    for node in ast.walk(ast.parse(text)):
        if isinstance(node, ast.Import):
            mods += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            mods.append(node.module or '')
    assert mods == ['numpy'], mods
    assert 'oracle' not in text
    assert 'np.sum' not in text and '.sum(' not in text                     # (the rule is a loop over bins in the stated order)


def test_struct_layout_matches_header(tmp_path):
    names = ['fields', 'min_bins', 'min_power', 'moments', 'count']
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "cosmo_pol_amd.h"\nint main(void) {\n'
                   'cpol_outputs o; memset(&o, 0, sizeof o);\n'
                   'printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(cpol_spectrum_moments), sizeof(cpol_outputs),\n'
                   '       offsetof(cpol_outputs, mask_sum8), offsetof(cpol_outputs, spectrum_moments), offsetof(cpol_outputs, member_stats),\n'
                   '       offsetof(cpol_outputs, superob), o.spectrum_moments == NULL, CPOL_SPECTRUM_MOMENTS_FIELDS);\n'
                   + ''.join('printf("%%zu %%zu\\n", offsetof(cpol_spectrum_moments, %s), sizeof(((cpol_spectrum_moments *)0)->%s));\n'
                             % (n, n) for n in names)
                   + 'return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    M, O = N.SpectrumMoments, N.Outputs
    want = [ctypes.sizeof(M), ctypes.sizeof(O), O.mask_sum8.offset, O.spectrum_moments.offset, O.member_stats.offset,
            O.superob.offset, 1, len(SM.FIELDS)]
    for n in names:
        want += [getattr(M, n).offset, getattr(M, n).size]
    assert got == want
    # ahead of member_stats, superob still last, off in a zero-initialised struct
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in O._fields_[-3:]] == ['spectrum_moments', 'member_stats', 'superob']
    assert O.spectrum_moments.offset == O.mask_sum8.offset + ptr and O.member_stats.offset == O.spectrum_moments.offset + ptr
    assert O.superob.offset + ptr == ctypes.sizeof(O)
    assert not O().spectrum_moments and not O().member_stats and not O().superob
    header = open(os.path.join(ROOT, 'include', 'cosmo_pol_amd.h')).read()
    assert 'spectrum_moments_rows' in header and 'Replaces in the reference: nothing (it forms no moment' in header


def test_the_library_exports_no_new_symbol():
    """the hook is a control name of cpol_debug_read: the version script and the binding's list of exports gain nothing"""
    text = open(os.path.join(ROOT, 'cosmo_pol_amd', 'csrc', 'exports.map')).read()
    assert 'moments' not in text
    assert not any('moment' in n for n in N.EXPORTS)
