"""Neighbourhood ensemble probabilities without a GPU: the rule (cosmo_pol_amd/neighbourhood.py: `ensemble_sums`) through its
own properties, the host helpers on a hand-made table, the Python refusals, the product object `EnsembleScores`, the ctypes
mirrors of cpol_fraction_probabilities and cpol_fractions against the header, and every refusal of the host plan
(cosmo_pol_amd/csrc/cpol_frac.h: frac_prob_check) through tests/c_host/frac_prob_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a program of its own.  All comparisons of sums are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import neighbourhood as NB
from cosmo_pol_amd import objects as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f4, u1, u4, u8 = np.float32, np.uint8, np.uint32, np.uint64
nan, inf = np.nan, np.inf
SUMS = ('diff2', 'forecast2', 'observed2')


def frac(n_y, n_x, thresholds, radii):
    return NB.Fractions(CP.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0)), 'ZH', thresholds, radii)


# ---------------------------------------------------------------------------------------------------- the rule's properties
@pytest.mark.parametrize('n_y, n_x', [(1, 1), (2, 3), (65, 67)])
def test_rule_properties(n_y, n_x):
    rng = np.random.default_rng(100 * n_y + n_x)
    pool = np.array([nan, -inf, inf, 0.0, -0.0, 0.5, 1.0, 1.0, 2.0, 3.5], dtype=f4)
    M = 5
    maps = rng.choice(pool, size=(M, n_y, n_x))
    obs = rng.choice(pool, size=(n_y, n_x))
    maps[:, 0, 0] = 3.5                                       # every member set at every finite threshold in one cell
    dom = (rng.random((n_y, n_x)) < 0.7).astype(u1)
    dom[0, 0] = 1
    spec = frac(n_y, n_x, [-inf, 0.5, 2.0], [0, 1, 4])
    for domain in (None, dom):
        n_domain = n_y * n_x if domain is None else int(domain.sum())
        inside = np.ones((n_y, n_x), bool) if domain is None else domain != 0
        res = NB.ensemble_sums(spec, maps, obs, domain)
        assert res['n_blocks'] == M and res['reliability'].shape == (3, 3, M + 1, 2) and res['reliability'].dtype == u8
        assert all(res[k].shape == (3, 3) and res[k].dtype == u8 for k in SUMS) and res['forecast2'].any()
        assert res['member_sum'].shape == res['member_any'].shape == (3, 3, n_y, n_x) and res['member_sum'].dtype == u4
        # one block: block b's row of `sums`
        for b in (0, M - 1):
            one, plain = NB.ensemble_sums(spec, maps[b], obs, domain), NB.sums(spec, maps[b:b + 1], obs, domain)
            for k in SUMS:
                assert np.array_equal(one[k], plain[k][0]), (b, k)
        # S at radius 0: the sum of the binary maps
        with np.errstate(invalid='ignore'):
            F = inside & (maps == maps)[:, None] & (maps[:, None] >= spec.thresholds[:, None, None])
        assert np.array_equal(res['member_sum'][:, 0], F.sum(axis=0).astype(u4))
        assert np.array_equal(res['member_any'][:, 0], F.sum(axis=0).astype(u4))
        # every reliability slice sums to n_domain
        assert (res['reliability'].sum(axis=(-2, -1)) == n_domain).all()
        # A <= M, and A == M where every member is set
        assert res['member_any'].max() <= M and (res['member_any'] <= res['member_sum']).all()
        assert (res['member_any'][1:, :, 0, 0] == M).all() and (res['member_any'][0][:, F[:, 0].all(axis=0)] == M).all()
        # the order of the blocks does not matter
        shuffled = NB.ensemble_sums(spec, maps[rng.permutation(M)], obs, domain)
        for k in SUMS + ('reliability', 'member_sum', 'member_any'):
            assert np.array_equal(shuffled[k], res[k]), k
        # a Probabilities is taken like its Fractions; fss reads the three sums unchanged
        again = NB.ensemble_sums(NB.Probabilities(spec, maps=True), maps, obs, domain)
        assert np.array_equal(again['diff2'], res['diff2']) and NB.fss(res).shape == (3, 3)
        # NEP and NMEP: S over the cells the window holds, A over M
        cells = NB.window_cells(spec, domain)
        assert cells.shape == (3, n_y, n_x) and (res['member_sum'] <= M * cells[None]).all()
        p = NB.nep(res, cells)
        assert np.nanmax(p) <= 1.0 and np.array_equal(np.isnan(p[0]), cells == 0)
        assert np.array_equal(NB.nmep(res), res['member_any'] / float(M))
    assert np.array_equal(NB.window_cells(spec)[1, 0, 0], min(2, n_y) * min(2, n_x))


def test_the_largest_one_row_case():
    """256 blocks all set on the longest one-row grid with a window of the whole row: every S is 256 * 1023."""
    n_x = 1023
    M, r = 256, 1023
    assert not NB.overflows(n_x, 1, M, r)
    spec = frac(1, n_x, [1.0], [r])
    maps, obs = np.full((M, 1, n_x), 2.0, f4), np.full((1, n_x), nan, f4)
    res = NB.ensemble_sums(spec, maps, obs)
    assert int(res['forecast2'][0, 0]) == n_x * (M * n_x) ** 2 == int(res['diff2'][0, 0]) and int(res['observed2'][0, 0]) == 0
    assert int(res['reliability'][0, 0, M, 0]) == n_x


# ---------------------------------------------------------------------------------------------------- the helpers, by hand
def test_brier_reliability_and_roc_by_hand():
    # M = 2, ten cells: k = 0: 4 no, 1 yes; k = 1: 1 no, 1 yes; k = 2: 1 no, 2 yes
    table = np.array([[4, 1], [1, 1], [1, 2]], u8).reshape(1, 1, 3, 2)
    res = {'reliability': table, 'n_blocks': 2}
    # (0 - 1)^2 * 1 + 0.25 * 1 + 0.25 * 1 + (1 - 0)^2 * 1 + 0 * 2 = 2.5 over ten cells
    assert NB.brier(res).shape == (1, 1) and NB.brier(res)[0, 0] == 0.25
    curve = NB.reliability_curve(res)
    assert curve['probability'].tolist() == [0.0, 0.5, 1.0] and curve['count'][0, 0].tolist() == [5, 2, 3]
    assert curve['observed_frequency'][0, 0].tolist() == [0.2, 0.5, 2.0 / 3.0]
    r = NB.roc(res)
    # at least 0, 1, 2, 3 of 2 members: hits 4, 3, 2, 0 of 4 observed; false alarms 6, 2, 1, 0 of 6 not observed
    assert r['pod'][0, 0].tolist() == [1.0, 0.75, 0.5, 0.0] and r['pofd'][0, 0].tolist() == [1.0, 2.0 / 6.0, 1.0 / 6.0, 0.0]
    area = (1.0 - 2.0 / 6.0) * (1.0 + 0.75) / 2 + (2.0 / 6.0 - 1.0 / 6.0) * (0.75 + 0.5) / 2 + (1.0 / 6.0) * 0.5 / 2
    assert abs(r['area'][0, 0] - area) < 1e-15
    # a perfect forecast: Brier 0, area 1; an empty table: NaN
    perfect = {'reliability': np.array([[7, 0], [0, 0], [0, 3]], u8).reshape(1, 1, 3, 2), 'n_blocks': 2}
    assert NB.brier(perfect)[0, 0] == 0.0 and NB.roc(perfect)['area'][0, 0] == 1.0
    assert np.isnan(NB.reliability_curve(perfect)['observed_frequency'][0, 0, 1])
    assert np.isnan(NB.brier({'reliability': np.zeros((1, 1, 3, 2), u8), 'n_blocks': 2})[0, 0])
    with pytest.raises(ValueError, match='member_sum'):
        NB.nep(res, np.ones((1, 1, 1)))
    with pytest.raises(ValueError, match='member_any'):
        NB.nmep(res)


# ---------------------------------------------------------------------------------------------------- Python refusals, the product
def attach(product, az, n_gates, n_members=None, take=None):
    structs, keep = product.attach(N, az, n_gates, n_members, True, True, ['U', 'V', 'W', 'T'], take)
    return structs, keep


def test_python_refusals_and_the_product_object():
    c = CP.Composite(['KDP', 'ZH'], [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0])            # a 2 x 3 grid
    spec = NB.Fractions(c, 'ZH', [0.5, 1.5], [0, 1, 4])
    with pytest.raises(ValueError, match='not built in Python'):
        NB.Probabilities(OB.Objects(spec))
    with pytest.raises(ValueError, match='neighbourhood.Fractions'):
        NB.Probabilities(c)
    with pytest.raises(ValueError, match='neighbourhood.Probabilities'):
        NB.EnsembleScores(spec)
    pr = NB.Probabilities(spec, maps=True)
    assert pr == NB.Probabilities(spec, maps=True) and pr != NB.Probabilities(spec) and hash(pr) == hash(NB.Probabilities(spec, maps=True))
    assert pr.composite is c and pr.radii is spec.radii and repr(pr).startswith('Probabilities(Fractions(')
    obs = np.arange(6, dtype=f4).reshape(2, 3)

    def take(block):
        return [np.zeros(sh, dt) for _, dt, sh in block], [0x77000 + 64 * i for i in range(len(block))]
    az4 = np.arange(4.0)
    p = NB.EnsembleScores(pr, obs, None, rays_per_block=2)
    assert isinstance(p, NB.Scores) and p.name == 'composite' and p.one_chunk
    structs, keep = attach(p, az4, 5, take=take)
    assert sorted(structs) == ['composite', 'fractions']
    f = structs['fractions']
    assert f.n_radii == 3 | N.FRAC_ENSEMBLE and not f.objects and isinstance(keep[-2], N.FractionsEnsemble)
    assert C.addressof(f) == C.addressof(keep[-2]) and (f.field, f.n_thresholds, f.observed) == (0, 2, 0x77000)
    assert p.arrays()[-5:] == [('sums', u8, (2, 2, 3, 3)), ('totals', u8, (2, 2, 3)), ('prob_sums', u8, (2, 3, 3)),
                               ('reliability', u8, (2, 3, 3, 2)), ('member_sum', u4, (2, 3, 2, 3))]
    for i, (path, _, _) in enumerate(p.arrays()):
        p.bind(path, 0x1000 * (i + 1))
    q = keep[-2].probabilities.contents
    n = len(p.arrays())
    assert (q.prob_sums, q.reliability, q.member_sum, q.member_any) == (0x1000 * (n - 2), 0x1000 * (n - 1), 0x1000 * n, None)
    assert (f.sums, f.totals) == (0x1000 * (n - 4), 0x1000 * (n - 3))
    # device outputs: the four entries beside the scores'; a map that was not asked for is refused like any unknown entry
    d = NB.EnsembleScores(NB.Probabilities(spec, any_maps=True))
    structs, keep = attach(d, az4, 5)
    d.bind_device({'count': 6, 'observed': 7, 'sums': 9, 'totals': 10, 'prob_sums': 11, 'reliability': 12, 'member_any': 13})
    q = keep[-2].probabilities.contents
    assert (q.prob_sums, q.reliability, q.member_sum, q.member_any) == (11, 12, None, 13) and structs['fractions'].sums == 9
    with pytest.raises(ValueError, match="unknown entry 'member_sum'"):
        d.bind_device({'member_sum': 1})
    # a call that does not finish the pass: no struct, no arrays
    p.phase = 1
    structs, keep = attach(p, az4, 5, take=take)
    assert sorted(structs) == ['composite'] and p.arrays() == []
    # the finish, and the join of one chunk; several chunks are refused
    p.phase = 3
    attach(p, az4, 5, take=take)
    views = {path: np.zeros(sh, dt) for path, dt, sh in p.arrays()}
    views['prob_sums'] = np.arange(3, dtype=u8)[None, None, :] * np.ones((2, 3, 3), u8)
    out = p.finish(views, None)
    pb = out['probabilities']
    assert sorted(pb) == sorted(SUMS + ('reliability', 'member_sum', 'n_blocks', 'thresholds', 'radii')) and pb['n_blocks'] == 2
    assert all((pb[k] == i).all() and pb[k].shape == (2, 3) for i, k in enumerate(SUMS)) and 'fractions' in out
    assert p.join([out], np.concatenate)['probabilities'] is pb
    with pytest.raises(ValueError, match='needs the members in one chunk'):
        p.join([out, out], np.concatenate)
    # more blocks than the table has rows for, and sums that could overflow: refused before the library sees the call
    with pytest.raises(ValueError, match='at most 256 blocks'):
        attach(NB.EnsembleScores(pr, obs, rays_per_block=1), np.arange(257.0), 5, take=take)
    big = frac(1023, 1023, [1.0], [1023])
    with pytest.raises(ValueError, match='could overflow'):
        attach(NB.EnsembleScores(NB.Probabilities(big), np.zeros((1023, 1023), f4), rays_per_block=1), np.arange(5.0), 5, take=take)
    with pytest.raises(ValueError, match='could overflow'):
        NB.ensemble_sums(big, np.zeros((5, 1023, 1023), f4), np.zeros((1023, 1023), f4))


def test_chunked_members_are_refused():
    """RadarOperator._ensemble_reduced: a member list cut into several chunks beside a Probabilities is a ValueError, before any
    call reaches the library."""
    from cosmo_pol_amd.radar_operator import RadarOperator

    class Stub(object):
        _members_arg = staticmethod(lambda members: [0, 1, 2])
        _ensemble_coords = staticmethod(lambda: (0.0, 0.0, 0.0))
        _cached = staticmethod(lambda key, make: type('Sub', (), {'n_sub': 1})())
        constants = type('K', (), {'RANGE_RADAR': np.arange(4.0)})()
        _lane = staticmethod(lambda lane: None)
        _set_plane = staticmethod(lambda *a: None)
        distributed = False

        def __init__(self, n_chunks):
            self.n_chunks, self.ran = n_chunks, []

        def _shared_member_chunks(self, ctx, members, n):
            return [members[i::self.n_chunks] for i in range(self.n_chunks)]

        def _run_rays(self, *a, **kw):
            self.ran.append(kw['members'])
            return {'n_sub': 1}
    spec = NB.Probabilities(NB.Fractions(CP.Composite(['ZH'], [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0]), 'ZH', [0.5], [0, 1]))
    obs = np.zeros((2, 3), f4)
    for per_member in (True, False):
        stub = Stub(2)
        product = RadarOperator._fss_product(stub, spec, obs, None, None, False, 3, 0)
        assert isinstance(product, NB.EnsembleScores)
        with pytest.raises(ValueError, match='needs the members in one chunk'):
            RadarOperator._ensemble_reduced(stub, [0.0, 1.0], [1.0, 1.0], product, 'maps', None, per_member, None, True, 0, False)
        assert stub.ran == []
    # one chunk goes through; a Fractions alone may still be cut
    stub = Stub(1)
    RadarOperator._ensemble_reduced(stub, [0.0, 1.0], [1.0, 1.0], product, 'maps', None, True, None, True, 0, False)
    assert stub.ran == [[0, 1, 2]]
    stub = Stub(2)
    plain = RadarOperator._fss_product(stub, spec.fractions, obs, None, None, False, 3, 0)
    assert type(plain) is NB.Scores
    with pytest.raises(ValueError, match='neighbourhood.Fractions'):
        RadarOperator._fss_product(stub, 'nonsense', obs, None, None, False, 3, 0)


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_struct_layouts_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){',
             'printf("cpol_fractions %zu\\n", sizeof(cpol_fractions));',
             'printf("cpol_fractions_ensemble %zu\\n", sizeof(cpol_fractions_ensemble));',
             'printf("cpol_fraction_probabilities %zu\\n", sizeof(cpol_fraction_probabilities));']
    for fname, _ in N.Fractions._fields_:
        lines.append('printf("f.%s %%zu\\n", offsetof(cpol_fractions, %s));' % (fname, fname))
    for fname, _ in N.FractionProbabilities._fields_:
        lines.append('printf("q.%s %%zu\\n", offsetof(cpol_fraction_probabilities, %s));' % (fname, fname))
    lines.append('printf("e.f %zu\\n", offsetof(cpol_fractions_ensemble, f));')
    lines.append('printf("e.probabilities %zu\\n", offsetof(cpol_fractions_ensemble, probabilities));')
    lines.append('printf("limit %d %d\\n", CPOL_FRAC_PROB_MAX_BLOCKS, CPOL_FRAC_ENSEMBLE);')
    lines.append('cpol_fractions_ensemble e; memset(&e, 0, sizeof e);')
    lines.append('printf("off %d\\n", e.probabilities == NULL && !(e.f.n_radii & CPOL_FRAC_ENSEMBLE)); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got['cpol_fractions']) == C.sizeof(N.Fractions)
    assert int(got['cpol_fraction_probabilities']) == C.sizeof(N.FractionProbabilities) == 32
    for fname, _ in N.Fractions._fields_:
        assert int(got['f.' + fname]) == getattr(N.Fractions, fname).offset, fname
    for fname, _ in N.FractionProbabilities._fields_:
        assert int(got['q.' + fname]) == getattr(N.FractionProbabilities, fname).offset, fname
    assert [f for f, _ in N.FractionProbabilities._fields_] == ['prob_sums', 'reliability', 'member_sum', 'member_any']
    # cpol_fractions keeps its size and its last member; the wrapper embeds it first, the pointer directly behind it, and a
    # zero-initialised wrapper means off: no flag, no pointer
    assert [f for f, _ in N.Fractions._fields_][-1] == 'objects' and got['off'] == '1'
    assert int(got['cpol_fractions_ensemble']) == C.sizeof(N.FractionsEnsemble) == C.sizeof(N.Fractions) + C.sizeof(C.c_void_p)
    assert int(got['e.f']) == N.FractionsEnsemble.f.offset == 0
    assert int(got['e.probabilities']) == N.FractionsEnsemble.probabilities.offset == C.sizeof(N.Fractions)
    assert [int(x) for x in got['limit'].split()] == [NB.MAX_PROB_BLOCKS, N.FRAC_ENSEMBLE] == [256, 0x10000]
    assert N.FRAC_PROB_MAX_BLOCKS == 256 and N.FRAC_ENSEMBLE > NB.MAX_RADII
    plain = N.Fractions()
    plain.n_radii, plain.field = 3, 5
    f, q, keep = N.Context.probabilities_struct(plain)
    assert (f.n_radii, f.field, plain.n_radii) == (3 | N.FRAC_ENSEMBLE, 5, 3) and C.addressof(f) == C.addressof(keep[0])
    assert C.addressof(keep[0].probabilities.contents) == C.addressof(q)
    assert not q.prob_sums and not q.reliability and not q.member_sum and not q.member_any


# ---------------------------------------------------------------------------------------------------- the host plan
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('frac_prob') / 'frac_prob_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'frac_prob_check.cpp'),
                        '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def run(exe, *calls):
    r = subprocess.run([exe] + list(calls), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls)
    out = []
    for line in lines:
        over, rest = line.split(' | ', 1)
        out.append((over == 'overflow 1', rest))
    return out


def plan(rest):
    assert rest.startswith('ok '), rest
    w = rest.split()
    return {name: int(x) for name, x in zip(w[1::2], w[2::2])}


def condition(n_x, n_y, M, r):
    """The condition of the rule in Python integers, written out here once more."""
    c = min(2 * r + 1, n_y) * min(2 * r + 1, n_x)
    return not (M * c < 2 ** 32 and n_y * n_x * (M * c) ** 2 < 2 ** 64)


def test_host_plan_accepts(exe):
    (over, rest), = run(exe, 'nx=300,ny=300,blocks=21,r=5,nthr=3,msum=1')
    p = plan(rest)
    groups = (300 * 300 + 1023) // 1024
    assert not over and p == {'on': 1, 'grid': 3 * 2 * groups, 'entries': 22 * 2, 'psums': 3 * 2 * 3 * 8, 'rel': 3 * 2 * 22 * 2 * 8,
                              'msum': 3 * 2 * 300 * 300 * 4, 'many': 0}
    (_, rest), = run(exe, 'nx=3,ny=2,blocks=1,r=0,many=1')
    assert plan(rest) == {'on': 1, 'grid': 1, 'entries': 4, 'psums': 24, 'rel': 32, 'msum': 0, 'many': 24}
    # without the flag, or with it and a NULL pointer: off, and nothing of it is planned (the outputs NULL, 300 blocks: not looked
    # at); NULL maps are "not wanted", not a refusal
    off = {'on': 0, 'grid': 0, 'entries': 0, 'psums': 0, 'rel': 0, 'msum': 0, 'many': 0}
    for call in ('prob=0', 'flag=0', 'flag=0,psums=0,rel=0', 'prob=0,flag=0'):
        (_, rest), = run(exe, 'nx=3,ny=2,blocks=300,r=1,' + call)
        assert plan(rest) == off, call
    # the flag is a flag only on a positive count: the counts the scores refuse stay refused, nothing behind the struct is read
    for nrad in (0, -1, -0x10000, 9, 0x10000, 0x10000 | 9, 0x20000 | 2):
        (_, rest), = run(exe, 'nx=3,ny=2,blocks=2,r=1,nrad=%d' % nrad)
        assert rest.startswith('refused n_radii must lie in 1 ... 8'), (nrad, rest)


def test_host_plan_refusals(exe):
    for call, word in (('psums=0', 'prob_sums or reliability is NULL'), ('rel=0', 'prob_sums or reliability is NULL'),
                       ('psums=0,rel=0', 'prob_sums or reliability is NULL'), ('blocks=257', 'at most 256 blocks'),
                       ('blocks=100000', 'at most 256 blocks')):
        (_, rest), = run(exe, 'nx=5,ny=4,' + call)
        assert rest.startswith('refused ') and word in rest, (call, rest)
    (_, ok), (_, no) = run(exe, 'nx=5,ny=4,blocks=256', 'nx=5,ny=4,blocks=257')
    assert plan(ok)['entries'] == 257 * 2 and plan(ok)['rel'] == 2 * 257 * 2 * 8 and no.startswith('refused ')
    # the refusals of cpol_fractions itself come first
    (_, rest), = run(exe, 'nx=0,ny=4,psums=0')
    assert rest.startswith('refused the maps need')


def test_host_plan_overflow_condition(exe):
    n = 1023
    # the four cases of the rule: (n_x, n_y, blocks, radius) -> refused?
    cases = [(300, 300, 21, 1023, False), (n, n, 128, 20, False), (n, n, 256, 32, False), (n, n, 128, 1023, True)]
    for n_x, n_y, M, r, refused in cases:
        assert condition(n_x, n_y, M, r) == refused == NB.overflows(n_x, n_y, M, r), (n_x, n_y, M, r)
        (over, rest), = run(exe, 'nx=%d,ny=%d,blocks=%d,r=%d' % (n_x, n_y, M, r))
        assert over == refused, (n_x, n_y, M, r, rest)
        # (the whole plan: 256 blocks of 1023^2 cells pass the condition and are refused by the 1 GiB of tables)
        if M == 256:
            assert '1 GiB' in rest
        else:
            assert rest.startswith('refused ') == refused and ('could overflow' in rest) == refused, rest
    # the first refused n_blocks at 1023^2 cells with radius 1023, and the last accepted one, through the whole plan
    first = next(M for M in range(1, 257) if condition(n, n, M, n))
    assert first == 5 and not condition(n, n, first - 1, n)
    (o_ok, ok), (o_no, no) = run(exe, 'nx=%d,ny=%d,blocks=%d,r=%d' % (n, n, first - 1, n), 'nx=%d,ny=%d,blocks=%d,r=%d' % (n, n, first, n))
    assert not o_ok and plan(ok)['on'] == 1 and o_no and 'could overflow' in no
    # both sides of the boundary in the radius, at 128 members
    r_first = next(r for r in range(0, 1024) if condition(n, n, 128, r))
    (o_ok, ok), (o_no, no) = run(exe, 'nx=%d,ny=%d,blocks=128,r=%d' % (n, n, r_first - 1), 'nx=%d,ny=%d,blocks=128,r=%d' % (n, n, r_first))
    assert r_first > 20 and not o_ok and plan(ok)['on'] == 1 and o_no and 'could overflow' in no
    # both sides on a one-row grid, where M * c < 2^32 always holds and the product decides ... never: 256 * 1023 squared times
    # 1023 is far below 2^64, so the longest one-row grid passes with every radius and block count
    assert not any(condition(n, 1, 256, r) for r in (0, 1, 511, 1023))
    (over, rest), = run(exe, 'nx=%d,ny=1,blocks=256,r=1023' % n)
    assert not over and plan(rest)['on'] == 1
    # the condition is decided on the numbers alone for block counts the plan refuses earlier: M * c >= 2^32 is the first clause
    M_big = next(M for M in (2 ** k for k in range(8, 40)) if M * n * n >= 2 ** 32)
    (over, rest), = run(exe, 'nx=%d,ny=%d,blocks=%d,r=%d' % (n, n, M_big, n))
    assert over and condition(n, n, M_big, n)
    # ... and huge numbers do not overflow the check itself
    (over, rest), = run(exe, 'nx=%d,ny=%d,blocks=%d,r=%d' % (n, n, 2 ** 31 - 1, n))
    assert over
