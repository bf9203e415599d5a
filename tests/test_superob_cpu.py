"""Superobservations without a GPU: superob.average against a plain-Python double loop written here from the rule's text,
the refusals, `shape`, the window coordinates, and the layout of cpol_superob / cpol_outputs against the header."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import superob as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = ['ZH', 'ZV', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V']


def loop_average(fields, R, G, frac, rpb):
    """The rule, gate by gate in Python floats (IEEE float64): {name: (values, counts)} as lists of lists."""
    n_rows, n_gates = fields['ZH'].shape
    rpb = rpb or n_rows
    wr, wc = -(-rpb // R), -(-n_gates // G)
    out = {}

    def window(b, i, j, arrays, gate_counts):
        """(sums of `arrays`, n, N) over one window"""
        S = [0.0] * len(arrays)
        n = N_ = 0
        for r in range(i * R, min((i + 1) * R, rpb)):
            s = [0.0] * len(arrays)
            for g in range(j * G, min((j + 1) * G, n_gates)):
                N_ += 1
                row = b * rpb + r
                if gate_counts(row, g):
                    n += 1
                    for a, x in enumerate(arrays):
                        s[a] = s[a] + float(x[row, g])
            for a in range(len(arrays)):
                S[a] = S[a] + s[a]
        return S, n, N_

    for k in list(fields) + ['ZDR']:
        if k == 'ZDR':
            arrays = [fields['ZH'], fields['ZV']]
            counts = lambda row, g: not math.isnan(fields['ZH'][row, g]) and not math.isnan(fields['ZV'][row, g])
            dt = np.float32
        else:
            arrays = [fields[k]]
            counts = lambda row, g, x=fields[k]: not math.isnan(x[row, g])
            dt = fields[k].dtype
        vals = np.empty(((n_rows // rpb) * wr, wc), dtype=dt)
        cnt = np.empty(vals.shape, dtype=np.uint16)
        for b in range(n_rows // rpb):
            for i in range(wr):
                for j in range(wc):
                    S, n, N_ = window(b, i, j, arrays, counts)
                    need = max(1, int(math.ceil(frac * N_)))
                    if n < need:
                        v = float('nan')
                    elif k == 'ZDR':
                        with np.errstate(all='ignore'):
                            v = np.float64(S[0]) / np.float64(S[1])
                    else:
                        v = S[0] / n
                    vals[b * wr + i, j] = v                  # (one rounding to the field's dtype)
                    cnt[b * wr + i, j] = n
        out[k] = (vals, cnt)
    return out


def random_fields(rng, n_rows, n_gates, nan_share=0.3):
    f = {}
    for k in F32 + ['RVEL']:
        dt = np.float64 if k == 'RVEL' else np.float32
        x = (rng.standard_normal((n_rows, n_gates)) * 10 ** rng.uniform(-3, 6)).astype(dt)
        if k in ('ZH', 'ZV'):
            x = np.abs(x)
        x[rng.random((n_rows, n_gates)) < nan_share] = np.nan          # (every field its own gaps: ZDR's gate set differs from ZH's)
        f[k] = x
    return f


def assert_same(got, want, tag):
    for k, (vals, cnt) in want.items():
        a, c = got[k], got['count'][k]
        assert a.dtype == vals.dtype and a.shape == vals.shape, (tag, k, a.dtype, a.shape, vals.shape)
        assert c.dtype == np.uint16 and np.array_equal(c, cnt), (tag, k)
        assert np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64)[~np.isnan(a)],
                              vals.view(np.uint32 if a.dtype == np.float32 else np.uint64)[~np.isnan(vals)]), (tag, k)
        assert np.array_equal(np.isnan(a), np.isnan(vals)), (tag, k)


# (n_rows, n_gates, R, G, fraction, rays_per_block)
SHAPES = [(7, 11, 1, 1, 1.0, 0), (7, 11, 1, 4, 0.5, 0), (7, 11, 3, 1, 0.5, 0), (7, 11, 3, 5, 0.3, 0), (7, 11, 9, 13, 0.3, 0),
          (8, 11, 3, 4, 0.5, 4), (8, 12, 2, 4, 1.0, 4), (6, 10, 2, 5, 0.3, 3), (5, 9, 2, 2, 0.7, 0)]


@pytest.mark.parametrize('n_rows,n_gates,R,G,frac,rpb', SHAPES)
def test_average_is_the_double_loop(n_rows, n_gates, R, G, frac, rpb):
    rng = np.random.default_rng(n_rows * 1000 + n_gates * 10 + R + G)
    f = random_fields(rng, n_rows, n_gates)
    spec = SO.Superob(R, G, frac)
    got = SO.average(f, spec, rays_per_block=rpb)
    want = loop_average(f, R, G, frac, rpb)
    assert_same(got, want, (n_rows, n_gates, R, G, frac, rpb))
    assert got['ZH'].shape == SO.shape(n_rows, n_gates, spec, rpb)
    # ZDR has its own gate set, and is not the quotient of the two superobservations
    assert (got['count']['ZDR'] != got['count']['ZH']).any()


def test_all_nan_window_need_and_fractions():
    # one row of windows of 1 x 10 gates: 0, 2, 3, 5, 10 valid gates
    x = np.full((1, 50), np.nan, dtype=np.float32)
    for w, n in enumerate([0, 2, 3, 5, 10]):
        x[0, w * 10:w * 10 + n] = np.float32(1.5) + np.arange(n, dtype=np.float32)
    f = {'ZH': x, 'ZV': x.copy()}
    for frac, alive in [(0.3, [0, 0, 1, 1, 1]), (0.5, [0, 0, 0, 1, 1]), (1.0, [0, 0, 0, 0, 1]), (0.21, [0, 0, 1, 1, 1]),
                        (0.2, [0, 1, 1, 1, 1]), (1e-9, [0, 1, 1, 1, 1])]:
        got = SO.average(f, SO.Superob(1, 10, frac))
        assert list((~np.isnan(got['ZH'][0])).astype(int)) == alive, frac        # exactly at `need` lives, one below does not
        assert list(got['count']['ZH'][0]) == [0, 2, 3, 5, 10]
        assert_same(got, loop_average(f, 1, 10, frac, 0), frac)
    # need counts the gates a PARTIAL window holds: 50 gates in windows of 20 -> the last holds 10
    got = SO.average(f, SO.Superob(1, 20, 0.5))
    assert got['ZH'].shape == (1, 3) and list(got['count']['ZH'][0]) == [2, 8, 10]
    assert list(np.isnan(got['ZH'][0])) == [True, True, False]


def test_windows_larger_than_the_call_and_identity():
    rng = np.random.default_rng(5)
    f = random_fields(rng, 3, 4)
    got = SO.average(f, SO.Superob(5, 9, 0.1))
    assert got['ZH'].shape == (1, 1)
    assert_same(got, loop_average(f, 5, 9, 0.1, 0), 'larger')
    one = SO.average(f, SO.Superob(1, 1, 1.0))
    for k in F32 + ['RVEL']:
        assert np.array_equal(one[k], f[k], equal_nan=True) and one[k].dtype == f[k].dtype, k
        assert np.array_equal(one['count'][k], (~np.isnan(f[k])).astype(np.uint16)), k


def test_signed_zero_and_member_axis():
    z = np.array([[-0.0, np.nan], [np.nan, -0.0]], dtype=np.float32)
    got = SO.average({'ZH': z}, SO.Superob(2, 2, 0.5))
    assert got['ZH'].view(np.uint32)[0, 0] == 0            # sums start from +0.0: +0.0 + -0.0 = +0.0
    rng = np.random.default_rng(9)
    f = random_fields(rng, 6, 7)
    three = {k: v.reshape(2, 3, 7) for k, v in f.items()}
    a = SO.average(three, SO.Superob(2, 3, 0.5))           # rays_per_block 0 = the rays of one member
    b = SO.average(f, SO.Superob(2, 3, 0.5), rays_per_block=3)
    for k in b:
        if k != 'count':
            assert a[k].shape == (2, 2, 3) and np.array_equal(a[k].reshape(b[k].shape), b[k], equal_nan=True), k


def test_refusals():
    for args in [(0, 1), (1, 0), (-1, 4), (256, 256), (65536, 1), (1.5, 2)]:
        with pytest.raises(ValueError):
            SO.Superob(*args)
    SO.Superob(255, 257)                                    # 65535: the largest window
    for frac in [0.0, -0.1, 1.0000001, float('nan'), float('inf')]:
        with pytest.raises(ValueError):
            SO.Superob(2, 2, frac)
    spec = SO.Superob(2, 2)
    f = {'ZH': np.zeros((6, 4), dtype=np.float32)}
    for rpb in (-1, 4, 7):
        with pytest.raises(ValueError):
            SO.average(f, spec, rays_per_block=rpb)
        with pytest.raises(ValueError):
            SO.shape(6, 4, spec, rpb)
    with pytest.raises(ValueError):
        SO.average({'mask': np.zeros((2, 2))}, spec)


def test_shape():
    assert SO.shape(360, 500, SO.Superob(4, 8)) == (90, 63)
    assert SO.shape(7, 11, SO.Superob(3, 5)) == (3, 3)
    assert SO.shape(8, 11, SO.Superob(3, 5), 4) == (4, 3)          # 3 + 1, 3 + 1 rays
    assert SO.shape(8, 11, SO.Superob(30, 50)) == (1, 1)


def test_coordinates_average_every_gate():
    rng = np.random.default_rng(3)
    geom = {'lats': rng.random((5, 7)), 'lons': rng.random((5, 7)), 'dist': rng.random((5, 7)).astype(np.float32),
            'heights': rng.random((5, 7)).astype(np.float32)}
    got = SO.coordinates(geom, SO.Superob(2, 3, 0.3))
    for k, v in geom.items():
        assert got[k].dtype == v.dtype and got[k].shape == (3, 3), k
        assert got[k][2, 2] == v[4, 6] and np.allclose(got[k][0, 0], v[:2, :3].mean(), rtol=1e-6), k


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cosmo_pol_amd.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(cpol_superob), sizeof(cpol_outputs), offsetof(cpol_outputs, superob),\n'
                   '       offsetof(cpol_superob, min_valid_fraction), offsetof(cpol_superob, ZH), offsetof(cpol_superob, count));\n'
                   'return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(N.Superob), ctypes.sizeof(N.Outputs), N.Outputs.superob.offset,
                   N.Superob.min_valid_fraction.offset, N.Superob.ZH.offset, N.Superob.count.offset]
    assert N.Outputs._fields_[-1][0] == 'superob'
    assert N.Outputs.superob.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(N.Outputs)
    assert not N.Outputs().superob                          # a zero-initialised struct: off
    assert [n for n, _ in N.Superob._fields_[5:]] == list(SO.FIELDS) + ['count'] == N.SUPEROB_FIELDS + ['count']
