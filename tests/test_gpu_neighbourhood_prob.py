"""Neighbourhood ensemble probabilities on the GPU, the kernels alone (k_frac_members behind k_frac_rows, k_frac_cols and
k_frac_score through cpol_debug_read "fractions_maps"): hand-built maps no sweep produces against neighbourhood.ensemble_sums of
the same maps.  Every intermediate is a count of integers, so every comparison is np.array_equal.  In each case the RULE's sums
are asserted not to be all zero first, so that an idle kernel cannot pass; the empty domain is the stated exception.  The hook
prefills every output with a poison value, which must be gone from every element."""
import numpy as np
import pytest

from test_gpu_composite import values
from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

f4, u1, u4, u8 = np.float32, np.uint8, np.uint32, np.uint64
inf = np.inf
SUMS = ('diff2', 'forecast2', 'observed2')
FSS_KEYS = SUMS + ('n_forecast', 'n_observed', 'n_domain')
POISON = 0xDEADBEEF
_ops = {}


def context():
    if 'op' not in _ops:
        conf, luts, cubes, _, _ = case('c2_rsg')
        op = operator(conf, luts)
        load(op, cubes[0])
        _ops['op'] = op
    return _ops['op']._ctx


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def NB():
    from cosmo_pol_amd import neighbourhood
    return neighbourhood


def spec_for(n_y, n_x, thresholds, radii):
    from cosmo_pol_amd import composite
    return NB().Fractions(composite.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0)), 'ZH', thresholds, radii)


class Wanted(object):
    def __init__(self, maps, any_maps):
        self.maps, self.any_maps = maps, any_maps


def assert_prob(got, want, which, tag):
    for k in SUMS + ('reliability',):
        assert got[k].dtype == u8 and got[k].shape == want[k].shape, (tag, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()), got[k].ravel()[:6], want[k].ravel()[:6])
    for k, on in (('member_sum', which.maps), ('member_any', which.any_maps)):
        assert (k in got) == on, (tag, k)
        if on:
            assert got[k].dtype == u4 and got[k].shape == want[k].shape, (tag, k)
            # (a count is at most 256 * 1023^2 < the poison value: equality with the rule says the prefill is gone from every element)
            assert not (got[k] == POISON).any() and np.array_equal(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()))
    assert got['n_blocks'] == want['n_blocks'], tag


def check(maps, obs, thresholds, radii, domain=None, which=(True, True), idle_allowed=False, tag=''):
    spec = spec_for(obs.shape[0], obs.shape[1], thresholds, radii)
    want, plain = NB().ensemble_sums(spec, maps, obs, domain), NB().sums(spec, maps, obs, domain)
    busy = all(want[k].any() for k in ('forecast2', 'reliability')) and (want['diff2'].any() or want['observed2'].any())
    assert busy != idle_allowed, (tag, 'the rule itself gives %s sums' % ('only zero' if not busy else 'non-zero'))
    which = Wanted(*which)
    got_plain, got = context().fractions_maps(maps, obs, spec, domain=domain, probabilities=which)
    assert_prob(got, want, which, tag)
    for k in FSS_KEYS:                                # the FSS sums beside it are what they were
        assert np.array_equal(got_plain[k], plain[k]), (tag, k)
    if idle_allowed:
        assert not any(got[k].any() for k in SUMS + ('reliability',)), tag
    return want


# (n_y, n_x): one cell; one row and one column of the longest grid; the smallest grid with both axes; rows and columns that
# cross the 64-lane chunks at non-multiples of 64; (65, 67) has more than four workgroups of 1024 cells per threshold
GRIDS = [(1, 1), (1, 1023), (1023, 1), (2, 3), (65, 67), (5, 130)]
ONE, FOUR = [0.75], [-inf, 0.0, 3.0, inf]
EIGHT = [0, 1, 2, 3, 5, 8, 64, 1023]


def drawn(rng, nb, n_y, n_x):
    """Maps and an observation out of the composite tests' pool: ties, NaN, both infinities, signed zeros, denormals; cell
    (0, 0) of block 0 and of the observation is set at every finite threshold used here, so no grid is too small to count."""
    maps, obs = values(rng, (nb, n_y, n_x)), values(rng, (n_y, n_x))
    maps[0, 0, 0] = 3.0
    obs[0, 0] = 3.0
    return maps, obs


@pytest.mark.parametrize('n_y, n_x', GRIDS)
def test_kernel_equals_the_rule(n_y, n_x):
    rng = np.random.default_rng(1000 * n_y + n_x)
    big = max(n_y, n_x)
    clip = sorted({1, max(1, min(n_y, n_x) // 2), max(2, big // 2), max(3, big - 1)})          # windows that reach every border
    part = (rng.random((n_y, n_x)) < 0.6).astype(u1)
    part[0, 0] = 1
    for nb in (1, 2, 3, 65):
        maps, obs = drawn(rng, nb, n_y, n_x)
        check(maps, obs, FOUR, clip, tag=('clipped at each border', nb, clip))
        check(maps, obs, FOUR, EIGHT[:5], domain=part, which=(True, False), tag=('a partial domain', nb))
        if nb in (1, 3):
            check(maps, obs, ONE, [min(big + 5, 1023)], which=(False, True), tag=('a radius larger than the grid', nb))
            check(maps, obs, FOUR, EIGHT, which=(False, False), tag=('eight radii, four thresholds', nb))
            check(maps, obs, ONE, [0, 2], domain=np.zeros((n_y, n_x), u1), idle_allowed=True, tag=('an empty domain', nb))
    # 256 blocks, the most the table holds: radii small enough for the condition on every grid here (256 * 17^2 cells a window)
    maps, obs = drawn(rng, 256, n_y, n_x)
    assert not NB().overflows(n_x, n_y, 256, 8)
    want = check(maps, obs, FOUR, [0, 1, 8], domain=part, tag='256 blocks')
    assert want['reliability'].shape[2] == 257


def test_one_block_is_the_fss_row_and_all_set_fills_the_last_row():
    rng = np.random.default_rng(7)
    maps, obs = drawn(rng, 1, 33, 70)
    spec = spec_for(33, 70, FOUR, [0, 2, 9])
    plain, got = context().fractions_maps(maps, obs, spec, probabilities=Wanted(False, False))
    for k in SUMS:
        assert got[k].any() and np.array_equal(got[k], plain[k][0]), k
    # every member set everywhere: A == M in every cell, the table's last row holds the whole domain
    full = np.full((5, 33, 70), 5.0, f4)
    want = check(full, obs, ONE, [0, 3], tag='all set')
    assert (want['member_any'] == 5).all() and (want['reliability'][..., 5, :].sum(axis=-1) == 33 * 70).all()


def test_with_an_empty_domain_the_maps_are_still_written():
    rng = np.random.default_rng(11)
    maps, obs = drawn(rng, 3, 9, 70)
    want = check(maps, obs, ONE, [0, 2], domain=np.zeros((9, 70), u1), idle_allowed=True, tag='an empty domain, both maps')
    assert want['member_sum'].shape == (1, 2, 9, 70) and not want['member_sum'].any()      # (nothing is set outside the domain)


def test_beside_objects():
    """cpol_objects and cpol_fraction_probabilities on one cpol_fractions: both results equal their rules, the FSS sums too."""
    from cosmo_pol_amd import objects as OB
    rng = np.random.default_rng(13)
    maps, obs = drawn(rng, 3, 21, 70)
    part = (rng.random((21, 70)) < 0.7).astype(u1)
    spec = spec_for(21, 70, FOUR, [0, 1, 4])
    ospec = OB.Objects(spec, connectivity=8, min_area=1, max_objects=256, labels=True)
    want, plain = NB().ensemble_sums(spec, maps, obs, part), NB().sums(spec, maps, obs, part)
    cells = OB.cells(ospec, maps, obs, part)
    assert want['forecast2'].any() and want['diff2'].any() and cells['n_objects'].any()
    which = Wanted(True, True)
    got_plain, got_cells, got = context().fractions_maps(maps, obs, spec, domain=part, objects=ospec, probabilities=which)
    assert_prob(got, want, which, 'beside objects')
    for k in FSS_KEYS:
        assert np.array_equal(got_plain[k], plain[k]), k
    alone = context().fractions_maps(maps, obs, spec, domain=part, objects=ospec)[1]
    for k in ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak', 'peak_cell', 'labels'):
        for a, b in ((got_cells[k], cells[k]), (got_cells[k], alone[k]), (got_cells['observed'][k], cells['observed'][k])):
            assert a.shape == b.shape and np.array_equal(a.view(u4), b.view(u4)), k       # ('peak': float32, bit for bit)


def test_refusals_leave_the_context_usable():
    rng = np.random.default_rng(3)
    maps, obs = drawn(rng, 2, 9, 11)
    spec = spec_for(9, 11, FOUR, [0, 3])
    ctx = context()
    both = Wanted(True, True)

    def null(name):
        return lambda f: setattr(f.probabilities, name, None)
    for tamper, what in ((null('prob_sums'), 'prob_sums or reliability'), (null('reliability'), 'prob_sums or reliability')):
        with pytest.raises(ValueError, match=what):
            ctx.fractions_maps(maps, obs, spec, tamper=tamper, probabilities=both)
        check(maps, obs, FOUR, [0, 3], tag=('after the refusal', what))
    # NULL maps are not a refusal: they are "not wanted"
    plain, got = ctx.fractions_maps(maps, obs, spec, tamper=null('member_sum'), probabilities=both)
    assert np.array_equal(got['diff2'], NB().ensemble_sums(spec, maps, obs)['diff2']) and (got['member_sum'] == POISON).all()
    # 257 blocks
    many = np.broadcast_to(maps[:1], (257, 9, 11))
    with pytest.raises(ValueError, match='at most 256 blocks'):
        ctx.fractions_maps(many, obs, spec, probabilities=both)
    ctx.fractions_maps(many, obs, spec)                   # (the scores alone take them, as before)
    check(maps, obs, FOUR, [0, 3], tag='after 257 blocks')
    # the overflow condition: 5 blocks of 1023 x 1023 cells with a window of the whole grid are the first refused, 4 pass
    n = 1023
    assert NB().overflows(n, n, 5, n) and not NB().overflows(n, n, 4, n)
    wide = spec_for(n, n, [1.0], [n])
    full, empty = np.full((5, n, n), 1.0, f4), np.full((n, n), np.nan, f4)
    with pytest.raises(ValueError, match='could overflow'):
        ctx.fractions_maps(full, empty, wide, probabilities=Wanted(False, False))
    check(maps, obs, FOUR, [0, 3], tag='after the overflow refusal')
    # ... and the last accepted side of the boundary: every S is 4 * 1023^2, and the sum 1023^2 * (4 * 1023^2)^2 passes 2^63
    plain, got = ctx.fractions_maps(full[:4], empty, wide, probabilities=Wanted(False, False))
    assert int(got['forecast2'][0, 0]) == n * n * (4 * n * n) ** 2 == int(got['diff2'][0, 0]) > 2 ** 63
    assert int(got['observed2'][0, 0]) == 0 and int(got['reliability'][0, 0, 4, 0]) == n * n
    assert int(got['reliability'].sum()) == n * n
