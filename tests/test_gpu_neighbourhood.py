"""Neighbourhood verification on the GPU, the kernels alone (k_frac_rows, k_frac_cols and k_frac_score through cpol_debug_read
"fractions_maps"): hand-built maps no sweep produces against neighbourhood.sums of the same maps.  Every intermediate is a count
of integers, so every comparison is np.array_equal on uint64.  In each case the RULE's sums are asserted not to be all zero
first, so that an idle kernel cannot pass; the empty-domain and none-set cases are the stated exceptions."""
import numpy as np
import pytest

from test_gpu_composite import values
from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

f4, u1, u8 = np.float32, np.uint8, np.uint64
inf = np.inf
KEYS = ('diff2', 'forecast2', 'observed2', 'n_forecast', 'n_observed', 'n_domain')
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


def check(maps, obs, thresholds, radii, domain=None, idle_allowed=False, tag=''):
    spec = spec_for(obs.shape[0], obs.shape[1], thresholds, radii)
    want = NB().sums(spec, maps, obs, domain)
    busy = any(want[k].any() for k in ('diff2', 'forecast2', 'observed2'))
    assert busy != idle_allowed, (tag, 'the rule itself gives %s sums' % ('only zero' if not busy else 'non-zero'))
    got = context().fractions_maps(maps, obs, spec, domain=domain)
    for k in KEYS:
        assert got[k].dtype == u8 and got[k].shape == want[k].shape, (tag, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()), got[k].ravel()[:6], want[k].ravel()[:6])
    return want


# (n_y, n_x): one cell; one row and one column of the longest grid; the smallest grid with both axes; rows and columns that
# cross the 64-lane chunks of k_frac_rows and k_frac_cols at non-multiples of 64, once and twice
GRIDS = [(1, 1), (1, 1023), (1023, 1), (2, 3), (65, 67), (130, 5), (5, 130)]
ONE, FOUR = [0.75], [-inf, 0.0, 3.0, inf]
EIGHT = [0, 1, 2, 3, 5, 8, 64, 1023]


def drawn(rng, nb, n_y, n_x):
    """Maps and an observation out of the composite tests' pool: ties, NaN, both infinities, signed zeros, denormals; cell
    (0, 0) of block 0 is set at every finite threshold used here, so no grid is too small for the rule to count something."""
    maps, obs = values(rng, (nb, n_y, n_x)), values(rng, (n_y, n_x))
    maps[0, 0, 0] = 3.0
    return maps, obs


@pytest.mark.parametrize('n_y, n_x', GRIDS)
def test_kernels_equal_the_rule(n_y, n_x):
    rng = np.random.default_rng(1000 * n_y + n_x)
    big = max(n_y, n_x)
    clip = sorted({1, max(1, min(n_y, n_x) // 2), max(2, big // 2), max(3, big - 1)})          # windows that reach every border
    for nb in (1, 3):
        maps, obs = drawn(rng, nb, n_y, n_x)
        part = (rng.random((n_y, n_x)) < 0.6).astype(u1)
        part[0, 0] = 1
        check(maps, obs, ONE, [0, 1], tag=('radii 0 and 1', nb))
        check(maps, obs, FOUR, clip, tag=('clipped at each border', nb, clip))
        check(maps, obs, ONE, [min(big + 5, 1023)], tag=('a radius larger than the grid', nb))
        check(maps, obs, FOUR, EIGHT, tag=('eight radii, four thresholds', nb))
        check(maps, obs, FOUR, EIGHT[:5], domain=part, tag=('a partial domain', nb))
        check(maps, obs, ONE, [0, 2], domain=np.zeros((n_y, n_x), u1), idle_allowed=True, tag=('an empty domain', nb))


@pytest.mark.parametrize('n_y, n_x', [(1, 1), (2, 3), (65, 67)])
def test_all_set_and_none_set_maps(n_y, n_x):
    full = np.full((3, n_y, n_x), 5.0, f4)
    full[1] = inf
    none = np.full((3, n_y, n_x), np.nan, f4)
    none[2] = -1.0                                               # (below the threshold everywhere)
    radii = [0, 1, 40, 200]
    want = check(full, full[0], ONE, radii, tag='all set against all set')
    assert not want['diff2'].any() and (want['n_forecast'] == n_y * n_x).all()
    # a window holds at most the whole grid: the largest count there is for this grid, in every cell
    assert (want['forecast2'][:, 0, -1] == (n_y * n_x) ** 3).all()
    check(full, none[0], ONE, radii, tag='all set against none set')
    check(none, full[0], ONE, radii, tag='none set against all set')
    check(none, none[0], ONE, radii, idle_allowed=True, tag='none set against none set')
    # with -inf as threshold every cell that is not NaN is set
    want = check(none, none[2], [-inf], radii, tag='-inf')
    assert want['n_forecast'].ravel().tolist() == [0, 0, n_y * n_x]


def test_the_largest_counts():
    """1023 x 1023 cells all set and a window of the whole grid: every count is 1023^2 and forecast2 = 1023^6 < 2^60, the
    largest sum the header's derivation allows; the observation empty, so diff2 is as large."""
    n = 1023
    full, empty = np.full((1, n, n), 1.0, f4), np.full((n, n), np.nan, f4)
    want = check(full, empty, [1.0], [0, 1023], tag='the largest sums')
    assert int(want['forecast2'][0, 0, 1]) == n ** 6 == int(want['diff2'][0, 0, 1]) and n ** 6 < 2 ** 60


def test_refusals_leave_the_context_usable():
    rng = np.random.default_rng(3)
    maps, obs = drawn(rng, 2, 9, 11)
    spec = spec_for(9, 11, FOUR, [0, 3])
    ctx = context()

    def set_to(name, value):
        def tamper(f):
            if isinstance(value, (list, tuple)):
                for j, v in enumerate(value):
                    getattr(f, name)[j] = v
            else:
                setattr(f, name, value)
        return tamper
    for tamper, what in ((set_to('n_thresholds', 0), 'n_thresholds'), (set_to('n_thresholds', 5), 'n_thresholds'),
                         (set_to('thresholds', [1.0, float('nan')]), 'NaN'), (set_to('n_radii', 0), 'n_radii'),
                         (set_to('n_radii', 9), 'n_radii'), (set_to('radii', [-1, 3]), 'radius'), (set_to('radii', [0, 1024]), 'radius'),
                         (set_to('radii', [3, 3]), 'ascending'), (set_to('observed', None), 'observed is NULL'),
                         (set_to('sums', None), 'sums or totals'), (set_to('totals', None), 'sums or totals')):
        with pytest.raises(ValueError, match=what):
            ctx.fractions_maps(maps, obs, spec, tamper=tamper)
        check(maps, obs, FOUR, [0, 3], tag=('after the refusal', what))
