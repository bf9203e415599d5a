"""The exact sums of the object cells without a GPU: `exact_sum` (integers alone) against math.fsum and fractions.Fraction on
finite bit patterns, denormals, cancellations and permutations; the host header (cosmo_pol_amd/csrc/cpol_obj.h) through
tests/c_host/obj_sums_check.cpp -- the split, the accumulator row and the hand rounding driven single-threaded, the bound case
included, built once plainly and once with the address and undefined-behaviour sanitizers as a program of its own --; the weight
function against composite.column_of; the grown cpol_objects against its ctypes mirror; every new refusal of obj_check; the
spec with the sums off; and `sal`, `weighted_centroids` and `zr_table` on cases whose results are exact.  Every comparison of
sums is on the bits."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import neighbourhood as NB
from cosmo_pol_amd import objects as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f4, f8, u1, u4, u8, i4 = np.float32, np.float64, np.uint8, np.uint32, np.uint64, np.int32
nan, inf = np.nan, np.inf
FLT_MAX = np.finfo(f4).max


def comp(n_x, n_y, **kw):
    return CP.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0), **kw)


def spec_of(n_x, n_y, thresholds, **kw):
    return OB.Objects(NB.Fractions(comp(n_x, n_y), 'ZH', thresholds, [0]), **kw)


def bits_of(x):
    return int(np.array([x], f8).view(u8)[0])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f8).view(u8), np.ascontiguousarray(b, f8).view(u8))


def to_float64(q):
    """The float64 nearest to the Fraction q, ties to even (Python's own correctly rounded division of integers)."""
    return q.numerator / q.denominator


def sets():
    """The summand sets: float32 arrays."""
    rng = np.random.default_rng(21)
    out = []
    for n in (1, 2, 3, 17, 300):
        raw = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(u4)
        raw = raw[((raw >> u4(23)) & u4(0xFF)) != 0xFF]                  # finite only
        out.append(raw.view(f4))
    out.append((rng.integers(0, 1 << 23, 40, dtype=np.uint64).astype(u4) | (rng.integers(0, 2, 40).astype(u4) << u4(31))).view(f4))     # denormals
    out.append(np.array([2.0 ** 100, 1.0, -2.0 ** 100], f4))
    out.append(np.array([FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX, 1e-45], f4))
    out.append(np.array([FLT_MAX] * 7 + [-FLT_MAX] * 7, f4))
    out.append(np.array([-0.0], f4))
    out.append(np.array([-0.0, 0.0, -0.0], f4))
    out.append(np.array([1.0, 2.0 ** -24, 2.0 ** -60], f4))                # a tie broken by the sticky rest
    out.append(np.array([1.0, 2.0 ** -53], f4))                          # a tie: to even (down)
    out.append(np.array([1.0 + 2.0 ** -23, 2.0 ** -53], f4))             # a tie with an odd last bit ... (53 bits: 1 + 2^-23 is even)
    out.append(np.array([2.0 ** 53, 1.0, 2.0], f4))                      # 2^53 + 3: a tie with an odd last bit, up
    out.append(np.array([], f4))
    return out


def test_exact_sum_against_fsum_and_fraction():
    rng = np.random.default_rng(22)
    for v in sets():
        for values in (v, v[rng.permutation(v.size)], v[::-1]):
            got = OB.exact_sum(values)
            assert bits_of(got) == bits_of(math.fsum(float(x) for x in values)), values
            assert bits_of(got) == bits_of(to_float64(sum((Fraction(float(x)) for x in values), Fraction(0)))), values
            # the weighted form: exact products with ix up to 1022
            ix = rng.integers(0, 1023, values.size)
            if values.size:
                ix[0] = 1022
            got = OB.exact_sum(values, ix)
            assert bits_of(got) == bits_of(math.fsum(float(x) * int(k) for x, k in zip(values, ix))), values
            assert bits_of(got) == bits_of(to_float64(sum((Fraction(float(x)) * int(k) for x, k in zip(values, ix)), Fraction(0)))), values
    assert bits_of(OB.exact_sum(np.array([-0.0], f4))) == 0 and bits_of(OB.exact_sum([])) == 0
    assert bits_of(OB.exact_sum(np.array([-1.5, -0.25], f4))) == bits_of(-1.75)
    for bad in ([inf], [1.0, nan], [-inf, 2.0]):
        with pytest.raises(ValueError, match='finite'):
            OB.exact_sum(np.array(bad, f4))
    with pytest.raises(ValueError, match='mult'):
        OB.exact_sum(np.array([1.0], f4), [1024])
    with pytest.raises(ValueError, match='mult'):
        OB.exact_sum(np.array([1.0], f4), [0.5])


def test_group_sums_equal_exact_sum():
    """The vectorised accumulator rows (what `cells` uses) against the literal integer sum, group by group."""
    rng = np.random.default_rng(23)
    raw = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(u4)
    raw[::97] = np.array([inf], f4).view(u4)[0]
    raw = raw[((raw >> u4(23)) & u4(0xFF) != 0xFF) | (raw & u4(0x7FFFFF) == 0)]           # no NaN
    w = raw.view(f4)
    ix, iy, g = rng.integers(0, 1023, w.size), rng.integers(0, 1023, w.size), rng.integers(0, 5, w.size)
    sums, skipped = OB.group_sums(w, ix, iy, g, 6)
    assert sums.shape == (6, 3) and skipped.dtype == u4 and skipped.sum() == np.isinf(w).sum() > 0
    for k in range(6):
        sel = (g == k) & np.isfinite(w)
        want = [OB.exact_sum(w[sel]), OB.exact_sum(w[sel], ix[sel]), OB.exact_sum(w[sel], iy[sel])]
        assert same_bits(sums[k], want) and skipped[k] == ((g == k) & np.isinf(w)).sum()
    assert same_bits(sums[5], [0.0, 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------- the host header
def build(tmp, name, extra):
    path = str(tmp / name)
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + extra +
                       ['-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'obj_sums_check.cpp'), '-o', path],
                       capture_output=True, text=True)
    return path, r


@pytest.fixture(scope='module')
def exes(tmp_path_factory):
    """The program built plainly and, where the compiler has the runtimes, once more with the sanitizers."""
    tmp = tmp_path_factory.mktemp('objsums')
    plain, r = build(tmp, 'obj_sums_check', [])
    assert r.returncode == 0, r.stderr
    out = [plain]
    san, r = build(tmp, 'obj_sums_check_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    if r.returncode == 0:
        out.append(san)
    else:
        assert 'sanitize' in r.stderr or 'asan' in r.stderr or 'ubsan' in r.stderr, r.stderr      # (only a missing runtime excuses it)
    return out


def run(exe, mode, *calls):
    r = subprocess.run([exe, mode] + list(calls), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls)
    return lines


def sum_file(path, w, ix, iy):
    with open(path, 'wb') as fh:
        np.array([w.size], i4).tofile(fh)
        np.ascontiguousarray(w, f4).view(u4).tofile(fh)
        np.ascontiguousarray(ix, i4).tofile(fh)
        np.ascontiguousarray(iy, i4).tofile(fh)
    return path


def test_host_build_of_split_bins_and_rounding(exes, tmp_path):
    rng = np.random.default_rng(24)
    files, want = [], []
    for v in sets():
        for values in (v, v[rng.permutation(v.size)]):
            ix, iy = rng.integers(0, 1023, values.size), rng.integers(0, 1023, values.size)
            files.append(sum_file(str(tmp_path / ('s%d.bin' % len(files))), values, ix, iy))
            want.append('ok %016x %016x %016x skipped 0' % tuple(bits_of(OB.exact_sum(values, k)) for k in (None, ix, iy)))
    # infinities are skipped, not summed
    v = np.array([1.0, inf, -inf, 2.0, inf], f4)
    files.append(sum_file(str(tmp_path / 'inf.bin'), v, [1, 2, 3, 4, 5], [0, 0, 0, 0, 9]))
    want.append('ok %016x %016x %016x skipped 3' % (bits_of(3.0), bits_of(9.0), bits_of(0.0)))
    # the bound case: 1023 x 1023 cells of FLT_MAX in one object.  No bin wraps, and the sums are the rule's
    yy, xx = np.indices((1023, 1023))
    big = np.full(1023 * 1023, FLT_MAX, f4)
    files.append(sum_file(str(tmp_path / 'big.bin'), big, xx.reshape(-1), yy.reshape(-1)))
    M = (1 << 24) - 1
    vol, mom = (M << 254) * 1023 * 1023, (M << 254) * 1023 * (1022 * 1023 // 2)
    want.append('ok %016x %016x %016x skipped 0' % (bits_of(OB.round_scaled(vol)), bits_of(OB.round_scaled(mom)), bits_of(OB.round_scaled(mom))))
    assert bits_of(OB.round_scaled(vol)) == bits_of(to_float64(Fraction(float(FLT_MAX)) * 1023 * 1023))
    files.append(sum_file(str(tmp_path / 'bigneg.bin'), -big, xx.reshape(-1), yy.reshape(-1)))
    want.append('ok %016x %016x %016x skipped 0' % (bits_of(-OB.round_scaled(vol)), bits_of(-OB.round_scaled(mom)), bits_of(-OB.round_scaled(mom))))
    for exe in exes:
        assert run(exe, 'sum', *files) == want
    # the vectorised rule on the bound case
    sums, skipped = OB.group_sums(big, xx.reshape(-1), yy.reshape(-1), np.zeros(big.size, np.int64), 1)
    assert ['%016x' % bits_of(q) for q in sums[0]] == want[-2].split()[1:4] and skipped[0] == 0


def test_weight_function_against_column_of(exes, tmp_path):
    """w = float32(f(m)): `weight_of` and the host build of obj_weight against composite.column_of's f, on and between the
    breakpoints, below and above the table."""
    rng = np.random.default_rng(25)
    for tv, tf in (OB.zr_table(), OB.zr_table(300.0, 1.4, 5.0, 55.0, 0.5), CP.vil_table(),
                   (np.array([1.0, 2.0], f4), np.array([0.25, 0.25])), (np.array([-3.0, 0.0, 0.5, 7.0, 9.0], f4), np.array([-2.0, -1.0, -1.0, 4.0, 1e300]))):
        assert tv.dtype == f4 and tf.dtype == f8 and np.all(tv[1:] > tv[:-1]) and np.all(tf[1:] >= tf[:-1])      # (zr_table is monotone)
        between = (tv[:-1].astype(f8) + rng.random(tv.size - 1) * (tv[1:].astype(f8) - tv[:-1])).astype(f4)
        v = np.concatenate([tv, between, np.nextafter(tv, f4(-inf)), np.nextafter(tv, f4(inf)),
                            np.array([tv[0] - 1, -inf, inf, tv[-1] * 2 + 1, -0.0, 0.0, 1e-42, FLT_MAX, -FLT_MAX], f4)]).astype(f4)
        # column_of with one layer of unit depth: the column IS f(m)
        if v.size % 2:
            v = np.append(v, f4(1.0))
        spec = CP.Composite(['ZH'], np.arange(v.size // 2 + 1.0), [0.0, 1.0, 2.0], products=('max', 'column'), z_edges=[0.0, 1.0], column={'ZH': (tv, tf)})
        col, _ = CP.column_of(spec, v.reshape(1, 1, 2, -1))
        with np.errstate(over='ignore'):
            want = col.reshape(-1).astype(f4)
        got = OB.weight_of(v, (tv, tf))
        assert got.dtype == f4 and np.array_equal(got.view(u4), want.view(u4))
        path = str(tmp_path / 'w.bin')
        with open(path, 'wb') as fh:
            np.array([tv.size, v.size], i4).tofile(fh)
            tv.tofile(fh)
            tf.tofile(fh)
            v.tofile(fh)
        for exe in exes:
            line, = run(exe, 'weight', path)
            assert line.split() == ['%08x' % b for b in want.view(u4)]
    assert np.isnan(OB.weight_of(np.array([nan, 1.0], f4), OB.zr_table())[0]) and OB.weight_of(np.array([3.0], f4)).view(u4)[0] == f4(3.0).view(u4)
    assert np.isinf(OB.weight_of(np.array([10.0], f4), (np.array([-3.0, 0.0, 0.5, 7.0, 9.0], f4), np.array([-2.0, -1.0, -1.0, 4.0, 1e300])))[0])
    tv, tf = OB.zr_table()
    assert tv.size == 241 and np.isclose(OB.weight_of(np.array([200.0], f4), (tv, tf))[0], 1.0, rtol=1e-3)       # Z = 200 R^1.6: 1 mm/h
    for kw, text in (({'a': 0.0}, 'a > 0'), ({'step_db': 0.01}, 'breakpoints'), ({'db_min': 70.0}, 'db_min < db_cap')):
        with pytest.raises(ValueError, match=text):
            OB.zr_table(**kw)


def test_obj_check_refusals_of_the_sums(exes):
    for exe in exes:
        got = run(exe, 'check', 'sums=0', 'sums=2', 'sums=-1', 'vol=0', 'skipped=0', 'field=0', 'cells=0', 'vol=4', 'field=4',
                  'nw=1', 'nw=1025', 'nw=-2', 'nw=4,wv=0', 'nw=4,wf=0', 'nw=4,tab=flat', 'nw=4,tab=desc', 'nw=4,tab=nan', 'nw=4,tab=inf',
                  'nx=1023,ny=1023,blocks=63,nthr=2,max=32', 'nx=1023,ny=1023,blocks=63,nthr=2,max=16')
        assert got[0].startswith('ok sums 0 scratch %d acc_offset 0 acc_bytes 0 ' % (2 * (2 * 6 + 2) * 4)) and got[0].endswith('volume 0 skipped 0 field 0 field_cells 0')
        assert got[1] == got[2] == 'refused sums must be 0 or 1'
        assert got[3] == got[4] == got[5] == got[6] == 'refused volume, skipped, field or field_cells is NULL'
        assert got[7] == got[8] == 'refused volume and field must be 8-byte aligned'
        assert got[9] == got[10] == got[11] == 'refused a weight table needs 2 ... 1024 breakpoints'
        assert got[12] == got[13] == 'refused weight_v or weight_f is NULL'
        assert got[14] == 'refused the breakpoints of the weight table are not strictly ascending'
        assert got[15] == 'refused the values of the weight table decrease'
        assert got[16] == got[17] == 'refused a breakpoint or a value of the weight table is NaN or infinite'
        # the labelling scratch alone passes (test_objects_cpu.py), the accumulators of 32 rows behind it do not; those of 16 do
        assert got[18] == 'refused the labelling scratch and the sums\' accumulators must be at most 1 GiB'
        assert got[19].startswith('ok sums 1 ')
        # the sizes of the measured case, against the Python mirror: 21 members and the observation, 300 x 300, three thresholds
        maps, cells, rows = 22 * 3, 90000, 1024
        label = maps * (2 * cells + 300) * 4
        line, = run(exe, 'check', 'nx=300,ny=300,blocks=21,nthr=3,max=1024,nw=241')
        acc = (maps * rows + 22) * 80 * 8
        assert line == 'ok sums 1 scratch %d acc_offset %d acc_bytes %d weight_offset %d finish %d volume %d skipped %d field %d field_cells %d' % (
            label + acc + 241 * 8 + 968, label, acc, label + acc, -(-(maps * rows + 22) * 3 // 256), maps * rows * 24, maps * rows * 4, 22 * 24, 22 * 8)
        spec = spec_of(300, 300, [1, 2, 3], sums=True, weight=OB.zr_table())
        assert OB.scratch_bytes(spec, 21) == label + acc + 241 * 8 + 968 and OB.SUM_BINS == 80
        # an odd number of labelling words: the accumulators on the next 8-byte boundary
        line, = run(exe, 'check', 'nx=1,ny=1,blocks=2,nthr=1,max=2')
        assert line.startswith('ok sums 1 scratch %d acc_offset 40 acc_bytes %d weight_offset %d ' % (40 + 9 * 640, 9 * 640, 40 + 9 * 640))
        assert OB.scratch_bytes(spec_of(1, 1, [1], sums=True, max_objects=2), 2) == 40 + 9 * 640


# ---------------------------------------------------------------------------------------------------- the C ABI and the spec
def test_grown_struct_matches_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){',
             'printf("cpol_objects %zu\\n", sizeof(cpol_objects));', 'printf("cpol_fractions %zu\\n", sizeof(cpol_fractions));']
    for fname, _ in N.Objects._fields_:
        lines.append('printf("o.%s %%zu\\n", offsetof(cpol_objects, %s));' % (fname, fname))
    lines.append('cpol_objects o; memset(&o, 0, sizeof o); printf("off %d\\n", o.sums == 0 && o.n_weight == 0 && o.volume == NULL);')
    lines.append('printf("table %d\\n", CPOL_COMP_MAX_TABLE); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got['cpol_objects']) == C.sizeof(N.Objects) == 96 and int(got['cpol_fractions']) == C.sizeof(N.Fractions)
    for fname, _ in N.Objects._fields_:
        assert int(got['o.' + fname]) == getattr(N.Objects, fname).offset, fname
    # the struct grew at its END: the old members lie where they lay, and a zero tail means off
    names = [n for n, _ in N.Objects._fields_]
    assert names == ['connectivity', 'min_area', 'max_objects', 'pad_', 'n_objects', 'table', 'labels', 'sums', 'n_weight', 'weight_v',
                     'weight_f', 'volume', 'skipped', 'field', 'field_cells']
    assert (N.Objects.labels.offset, N.Objects.sums.offset) == (32, 40) and got['off'] == '1' and N.Objects().sums == 0
    assert int(got['table']) == OB.MAX_TABLE == CP.MAX_TABLE


def test_spec_with_the_sums_off_is_todays():
    fr = NB.Fractions(comp(4, 3), 'ZH', [0.1], [1, 2])
    a = OB.Objects(fr, sums=False)
    assert a.key == (fr.key, 4, 1, 1024, True) and a == OB.Objects(fr) and (a.sums, a.weight) == (False, None)
    assert repr(a) == 'Objects(%r, connectivity=4, min_area=1, max_objects=1024, labels=True)' % (fr,)
    assert OB.scratch_bytes(a, 2) == 3 * (2 * 12 + 3) * 4
    tab = OB.zr_table()
    b, c = OB.Objects(fr, sums=True), OB.Objects(fr, sums=True, weight=tab)
    assert len({a, b, c}) == 3 and c == OB.Objects(fr, sums=True, weight=OB.zr_table()) and c != OB.Objects(fr, sums=True, weight=OB.zr_table(b=1.5))
    assert repr(b).endswith('labels=True, sums=True)') and repr(c).endswith('sums=True, weight=<241 breakpoints>)')
    assert c.weight[0].dtype == f4 and c.weight[1].dtype == f8
    for weight, text in ((tab, 'belongs to sums=True'),):
        with pytest.raises(ValueError, match=text):
            OB.Objects(fr, weight=weight)
    for weight, text in ((3, r'\(table_v, table_f\)'), (([1.0], [1.0]), '2 ... 1024 breakpoints'), (([1.0, 2.0], [1.0]), '2 ... 1024 breakpoints'),
                         (([1.0, 1.0], [1.0, 2.0]), 'strictly ascending'), (([1.0, 2.0], [2.0, 1.0]), 'decrease'),
                         (([1.0, 2.0], [nan, 1.0]), 'NaN or infinite'), (([1.0, inf], [0.0, 1.0]), 'NaN or infinite'),
                         (([1.0, 1e39], [0.0, 1.0]), 'NaN or infinite')):
        with pytest.raises(ValueError, match=text):
            OB.Objects(fr, sums=True, weight=weight)


def attach(product, az, n_gates, n_members=None, take=None):
    return product.attach(N, az, n_gates, n_members, True, True, ['U', 'V', 'W', 'T'], take)[0]


def test_cells_product_carries_the_sums():
    def take(block):
        return [np.zeros(sh, dt) for _, dt, sh in block], [0x77000 + 64 * i for i in range(len(block))]
    fr = NB.Fractions(comp(3, 2), 'ZH', [0.5, 1.5], [0])
    obs = np.arange(6, dtype=f4).reshape(2, 3)
    az4 = np.arange(4.0)
    off = OB.Cells(OB.Objects(fr, max_objects=5), obs, rays_per_block=2)
    o = attach(off, az4, 5, take=take)['fractions'].objects.contents
    assert [k for k, _, _ in off.arrays()][-3:] == ['n_objects', 'table', 'labels']
    assert (o.sums, o.n_weight, o.weight_v, o.volume, o.skipped, o.field, o.field_cells) == (0, 0, None, None, None, None, None)
    tab = OB.zr_table()
    p = OB.Cells(OB.Objects(fr, max_objects=5, sums=True, weight=tab), obs, rays_per_block=2)
    structs = attach(p, az4, 5, take=take)
    o = structs['fractions'].objects.contents
    assert (o.sums, o.n_weight) == (1, 241) and o.weight_v and o.weight_f
    assert p.arrays()[-4:] == [('volume', f8, (3, 2, 5, 3)), ('skipped', u4, (3, 2, 5)), ('field', f8, (3, 3)), ('field_cells', u4, (3, 2))]
    assert p.arrays()[:-4] == off.arrays()
    for i, (path, _, _) in enumerate(p.arrays()):
        p.bind(path, 0x1000 * (i + 1))
    n = len(p.arrays())
    assert (o.volume, o.skipped, o.field, o.field_cells) == tuple(0x1000 * (n - 3 + k) for k in range(4))
    d = OB.Cells(OB.Objects(fr, sums=True))
    o = attach(d, az4, 5)['fractions'].objects.contents
    d.bind_device({'n_objects': 11, 'table': 16, 'volume': 24, 'skipped': 28, 'field': 32, 'field_cells': 36})
    assert (o.sums, o.n_weight, o.volume, o.skipped, o.field, o.field_cells) == (1, 0, 24, 28, 32, 36)
    # the finish names the new arrays; the join stacks them, the field's too
    views = {path: np.zeros(sh, dt) for path, dt, sh in p.arrays()}
    views['volume'] = np.arange(3.0) * np.ones((3, 2, 5, 3))
    views['field'] = np.arange(9.0).reshape(3, 3)
    views['field_cells'] = np.arange(6, dtype=u4).reshape(3, 2)
    out = p.finish(dict(views), None)
    ob = out['objects']
    assert (ob['volume'] == 0).all() and (ob['moment_x'] == 1).all() and (ob['moment_y'] == 2).all() and ob['volume'].shape == (2, 2, 5)
    assert ob['skipped'].shape == (2, 2, 5) and ob['skipped'].dtype == u4 and ob['observed']['moment_y'].shape == (2, 5)
    assert sorted(ob['field']) == ['cells', 'moment_x', 'moment_y', 'skipped', 'volume'] and ob['field']['moment_x'].tolist() == [1.0, 4.0]
    assert ob['observed']['field']['volume'] == 6.0 and ob['field']['cells'].tolist() == [0, 2] and ob['observed']['field']['skipped'] == 5
    assert ob['weight'][0] is p.spec.weight[0] and ob['grid'] == (2, 3)
    j = p.join([out, out], np.concatenate)['objects']
    assert j['volume'].shape == (4, 2, 5) and j['skipped'].shape == (4, 2, 5) and j['field']['moment_x'].tolist() == [1.0, 4.0, 1.0, 4.0]
    assert j['field']['cells'].shape == (4,) and j['observed'] is ob['observed'] and j['weight'] is ob['weight'] and j['grid'] == (2, 3)
    big = OB.Objects(NB.Fractions(comp(1023, 1023), 'ZH', [1, 2], [0]), max_objects=32, sums=True)
    with pytest.raises(ValueError, match='labelling scratch and the sums of 63 blocks need more than 1 GiB'):
        attach(OB.Cells(big, np.zeros((1023, 1023), f4), rays_per_block=1), np.arange(63.0), 5, take=take)
    small = OB.Objects(big.fractions, max_objects=16, sums=True)
    attach(OB.Cells(small, np.zeros((1023, 1023), f4), rays_per_block=1), np.arange(63.0), 5, take=take)


# ---------------------------------------------------------------------------------------------------- cells, sal, centroids
def test_cells_sums_against_fsum():
    rng = np.random.default_rng(26)
    pool = np.array([nan, -inf, inf, 0.0, -0.0, 0.5, 1.0, -1.0, 2.0 ** 100, -2.0 ** 100, 3.5, 1e-42, FLT_MAX, -FLT_MAX, 1e-30], dtype=f4)
    maps = pool[rng.integers(0, len(pool), (2, 9, 11))]
    obs = pool[rng.integers(0, len(pool), (9, 11))]
    dom = (rng.random((9, 11)) < 0.85).astype(u1)
    off = OB.cells(spec_of(11, 9, [-inf, 0.0, 1.0, inf], connectivity=8, max_objects=4), maps, obs, dom)
    res = OB.cells(spec_of(11, 9, [-inf, 0.0, 1.0, inf], connectivity=8, max_objects=4, sums=True), maps, obs, dom)
    new = {'volume', 'moment_x', 'moment_y', 'skipped', 'field'}
    assert set(res) - set(off) == new | {'weight', 'grid'} and set(res['observed']) - set(off['observed']) == new and res['weight'] is None
    yy, xx = np.indices((9, 11))
    some = 0
    for s in range(3):
        side, v = (res, maps[s]) if s < 2 else (res['observed'], obs)
        part = (lambda k: side[k][s]) if s < 2 else (lambda k: side[k])
        sel = (dom != 0) & (v == v)
        fin = sel & np.isfinite(v)
        fld = {k: (q[s] if s < 2 else q) for k, q in side['field'].items()}
        assert (fld['cells'], fld['skipped']) == (fin.sum(), (sel & ~fin).sum())
        assert bits_of(fld['volume']) == bits_of(math.fsum(v[fin].astype(f8)))
        assert bits_of(fld['moment_x']) == bits_of(math.fsum(v[fin].astype(f8) * xx[fin]))
        for t in range(4):
            lab = part('labels')[t]
            for k in range(4):
                cellsk = (lab == k + 1) & np.isfinite(v)
                want = [math.fsum(v[cellsk].astype(f8)), math.fsum(v[cellsk].astype(f8) * xx[cellsk]), math.fsum(v[cellsk].astype(f8) * yy[cellsk])]
                got = [part('volume')[t, k], part('moment_x')[t, k], part('moment_y')[t, k]]
                assert [bits_of(q) for q in got] == [bits_of(q) for q in want], (s, t, k)
                assert part('skipped')[t, k] == ((lab == k + 1) & np.isinf(v)).sum()
                some += want[0] != 0
    assert some > 8


def sal_case(m, o, **kw):
    spec = spec_of(m.shape[-1], m.shape[-2], [1.0], sums=True, **kw)
    return OB.cells(spec, m.astype(f4), o.astype(f4))


def test_sal_and_weighted_centroids_on_exact_cases():
    o = np.zeros((12, 16))
    o[2:6, 3:7] = 4.0
    o[3, 4] = 8.0
    o[8:10, 10:14] = 2.0
    d = float(np.sqrt(np.float64(16 * 16 + 12 * 12)))
    # identical maps
    r = OB.sal(sal_case(o[None], o))
    assert all(r[k].shape == (1,) and r[k][0] == 0.0 for k in ('S', 'A', 'L', 'L1', 'L2'))
    # forecast = 2 x observed, powers of two: A = 2/3 computed the same way, S = 0, L = 0
    res = sal_case(np.stack([2 * o, o]), o)
    r = OB.sal(res)
    D = res['observed']['field']['volume'] / res['observed']['field']['cells']
    assert r['A'][0] == (2 * D - D) / (0.5 * (2 * D + D)) and r['A'][1] == 0.0 and (r['S'] == 0.0).all() and (r['L'] == 0.0).all()
    assert res['observed']['field']['cells'] == 192 and res['field']['volume'][0] == 2 * (16 * 4.0 + 4.0 + 8 * 2.0)
    # one square object shifted by k cells (the rest NaN: no field but the object): L1 = k / d, L2 = 0
    sq = np.full((12, 16), nan)
    sq[4:8, 2:6] = 1.0
    for k in (1, 3, 9):
        res = sal_case(np.roll(sq, k, axis=1)[None], sq)
        r = OB.sal(res)
        assert r['L1'][0] == k / d and r['L2'][0] == 0.0 and r['L'][0] == k / d and r['A'][0] == 0.0 and r['S'][0] == 0.0
        assert OB.sal(res, d=2.0)['L1'][0] == k / 2.0
        c = OB.weighted_centroids(res)
        assert c.shape == (1, 1, 1024, 2) and c[0, 0, 0].tolist() == [4.0 + k, 6.0] and np.isnan(c[0, 0, 1:]).all()
        assert OB.weighted_centroids(res['observed'])[0, 0].tolist() == [4.0, 6.0]
    # the weighted centroid is pulled to the heavy cell; a zero volume gives NaN
    m = np.zeros((1, 4))
    m[0] = [1.0, 1.0, 1.0, 5.0]
    res = OB.cells(spec_of(4, 1, [-1.0, 1.0], sums=True, max_objects=2), m.astype(f4), np.array([[1.0, -1.0, 0.0, 0.0]], f4))
    assert OB.weighted_centroids(res)[0, 1, 0].tolist() == [(0 + 1 + 2 + 15) / 8 + 0.5, 0.5] and OB.centroids(res)[0, 1, 0].tolist() == [2.0, 0.5]
    assert np.isnan(OB.weighted_centroids(res['observed'])[0, 0]).all() and res['observed']['area'][0, 0] == 4
    # no object on one side: NaN (A and L1 need the fields alone)
    r = OB.sal(sal_case(np.zeros((1, 12, 16)), o))
    assert np.isnan(r['S'][0]) and np.isnan(r['L2'][0]) and np.isnan(r['L'][0]) and r['A'][0] == -2.0 and np.isnan(r['L1'][0])
    r = OB.sal(sal_case(o[None], np.full((12, 16), nan)))
    assert all(np.isnan(r[k][0]) for k in ('S', 'A', 'L', 'L1', 'L2'))
    # more objects than table rows: the entries that need the objects are NaN, the others stand
    r = OB.sal(sal_case(o[None], o, max_objects=1))
    assert np.isnan(r['S'][0]) and np.isnan(r['L2'][0]) and np.isnan(r['L'][0]) and r['A'][0] == 0.0 and r['L1'][0] == 0.0
    # under a weight table S uses w(peak)
    tab = (np.array([0.0, 16.0], f4), np.array([0.0, 4.0]))
    res = OB.cells(spec_of(16, 12, [1.0], sums=True, weight=tab), np.stack([2 * o, o]).astype(f4), o.astype(f4))
    assert res['observed']['volume'][0, 0] == 16 * 1.0 + 1.0 and res['volume'][0, 0, 0] == 2 * 17.0 and OB.sal(res)['S'].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError, match='no exact sums'):
        OB.sal(OB.cells(spec_of(16, 12, [1.0]), o.astype(f4), o.astype(f4)))
    with pytest.raises(ValueError, match='threshold index'):
        OB.sal(res, threshold=1)
