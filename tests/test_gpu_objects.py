"""Object cells on the GPU, the kernels alone (k_obj_* behind k_frac_score through cpol_debug_read "fractions_maps"): hand-built
maps no sweep produces against objects.cells of the same maps.  Every attribute is a count, an integer sum, an integer extreme
or a comparison, so every comparison is np.array_equal.  In each case the RULE is asserted to find at least one object first, and
in the merge cases more row runs than objects, so that an idle kernel cannot pass.  The scores of the same call are compared with
neighbourhood.sums too: the cells change nothing of them."""
import numpy as np
import pytest

from _objects import PATTERNS, SHAPES, pattern
from test_gpu_composite import values
from test_gpu_ensemble import case, load, operator

pytestmark = pytest.mark.gpu

f4, u1, u4, i4 = np.float32, np.uint8, np.uint32, np.int32
inf, nan = np.inf, np.nan
KEYS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')
SUMS = ('diff2', 'forecast2', 'observed2', 'n_forecast', 'n_observed', 'n_domain')
ONE, FOUR = [0.75], [-inf, 0.0, 3.0, inf]
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


def mods():
    from cosmo_pol_amd import neighbourhood, objects
    return neighbourhood, objects


def spec_for(n_y, n_x, thresholds, **kw):
    from cosmo_pol_amd import composite
    NB, OB = mods()
    return OB.Objects(NB.Fractions(composite.Composite(['ZH'], np.arange(n_x + 1.0), np.arange(n_y + 1.0)), 'ZH', thresholds, [0]), **kw)


def same(got, want, tag):
    for k in KEYS:
        assert got[k].dtype == u4 and got[k].shape == want[k].shape, (tag, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()), got[k].ravel()[:8], want[k].ravel()[:8])
    assert got['peak'].dtype == f4 and np.array_equal(got['peak'].view(u4), want['peak'].view(u4)), (tag, 'peak')
    assert ('labels' in got) == ('labels' in want), tag
    if 'labels' in want:
        assert got['labels'].dtype == i4 and got['labels'].shape == want['labels'].shape, (tag, 'labels')
        assert np.array_equal(got['labels'], want['labels']), (tag, 'labels', int((got['labels'] != want['labels']).sum()))


def check(maps, obs, thresholds, domain=None, merges=False, idle_allowed=False, tag='', **kw):
    NB, OB = mods()
    maps = maps if maps.ndim == 3 else maps[None]
    spec = spec_for(obs.shape[0], obs.shape[1], thresholds, **kw)
    want = OB.cells(spec, maps, obs, domain)
    found = int(want['n_objects'].sum()) + int(want['observed']['n_objects'].sum())
    assert (found > 0) != idle_allowed, (tag, 'the rule itself finds %d objects' % found)
    if merges:
        F, O, _, _ = OB.binary_maps(spec.fractions, maps, obs, domain)
        runs = sum(len(OB._runs(b)[0]) for b in list(F.reshape((-1,) + obs.shape)) + list(O))
        objects = sum(OB.label(b, spec.connectivity)[1] for b in list(F.reshape((-1,) + obs.shape)) + list(O))
        assert runs > objects, (tag, 'no merge in this case', runs, objects)
    sums, got = context().fractions_maps(maps, obs, spec.fractions, domain=domain, objects=spec)
    same(got, want, tag)
    same(got['observed'], want['observed'], (tag, 'observed'))
    assert (got['connectivity'], got['min_area']) == (spec.connectivity, spec.min_area) and np.array_equal(got['thresholds'], spec.thresholds)
    want_sums = NB.sums(spec.fractions, maps, obs, domain)
    for k in SUMS:
        assert np.array_equal(sums[k], want_sums[k]), (tag, k)
    if spec.min_area == 1 and int(want['n_objects'].max()) <= spec.max_objects and int(want['observed']['n_objects'].max()) <= spec.max_objects:
        # the invariant: every set cell lies in exactly one object
        assert np.array_equal(got['area'].sum(axis=-1, dtype=np.uint64), sums['n_forecast']), (tag, 'sum of areas')
        assert np.array_equal(got['observed']['area'].sum(axis=-1, dtype=np.uint64), sums['n_observed'][0]), (tag, 'sum of areas, observed')
    return want


def field(binary, rng=None):
    """float32 values whose cells >= 0.75 are those of `binary`; with rng: distinct-ish values, so that the peaks differ."""
    hi = np.full(binary.shape, 5.0, f4) if rng is None else (1.0 + rng.integers(0, 50, binary.shape)).astype(f4)
    return np.where(binary, hi, f4(-1.0)).astype(f4)


def test_one_cell_set_and_unset():
    one, none = np.full((1, 1), 2.0, f4), np.full((1, 1), nan, f4)
    for connectivity in (4, 8):
        want = check(one, none, ONE, connectivity=connectivity, tag='set against unset')
        assert want['n_objects'].tolist() == [[1]] and want['observed']['n_objects'].tolist() == [0]
        check(none, one, ONE, connectivity=connectivity, tag='unset against set')
        check(none, none, ONE, connectivity=connectivity, idle_allowed=True, tag='both unset')


@pytest.mark.parametrize('n_y, n_x', SHAPES)
@pytest.mark.parametrize('connectivity', [4, 8])
def test_patterns_equal_the_rule(n_y, n_x, connectivity):
    rng = np.random.default_rng(100 * n_y + n_x)
    maps = np.stack([field(pattern(name, (n_y, n_x)), rng) for name in PATTERNS])
    for k in range(0, len(PATTERNS), 3):                  # three blocks and the observation in one call
        check(maps[k:k + 3], maps[(k + 3) % len(PATTERNS)], ONE, connectivity=connectivity, merges=n_y > 1 and n_x > 1,
              max_objects=4096, tag=PATTERNS[k:k + 3])


def test_checkerboard_and_comb_counts():
    board, comb = pattern('checkerboard', (65, 67)), pattern('comb', (65, 67))
    want = check(np.stack([field(board), field(comb)]), field(pattern('serpentine', (65, 67))), ONE, connectivity=4, merges=True,
                 max_objects=4096, tag='4')
    assert want['n_objects'].ravel().tolist() == [int(board.sum()), 1] and want['observed']['n_objects'].tolist() == [1]
    assert want['observed']['area'][0, 0] == 33 * 67 + 32
    want = check(np.stack([field(board), field(comb)]), field(pattern('spiral', (65, 67))), ONE, connectivity=8, merges=True, tag='8')
    assert want['n_objects'].ravel().tolist() == [1, 1]


@pytest.mark.parametrize('n_y, n_x', SHAPES)
def test_value_classes_thresholds_domain_and_nan(n_y, n_x):
    """Three blocks plus the observation at four thresholds in one call, out of the composite tests' pool: ties, NaN, both
    infinities, signed zeros, denormals; then a domain mask that cuts objects in two."""
    rng = np.random.default_rng(1000 * n_y + n_x)
    maps, obs = values(rng, (3, n_y, n_x)), values(rng, (n_y, n_x))
    maps[0, 0, 0] = 3.0
    part = (rng.random((n_y, n_x)) < 0.7).astype(u1)
    part[0, 0] = 1
    for connectivity in (4, 8):
        check(maps, obs, FOUR, connectivity=connectivity, max_objects=2048, tag=('pool', connectivity))
        check(maps, obs, FOUR, domain=part, connectivity=connectivity, max_objects=2048, tag=('pool, domain', connectivity))
    check(maps, obs, FOUR, domain=np.zeros((n_y, n_x), u1), idle_allowed=True, tag='an empty domain')


def test_an_object_cut_in_two_by_the_domain():
    full = np.full((9, 70), 4.0, f4)
    dom = np.ones((9, 70), u1)
    dom[:, 64] = 0                                        # (the cut lies at a chunk border)
    want = check(full, full, ONE, domain=dom, connectivity=8, merges=True, tag='cut')
    assert want['n_objects'].tolist() == [[2]] and want['area'][0, 0, :2].tolist() == [9 * 64, 9 * 5]
    full[4, :] = nan                                      # ... and a row of NaN cuts both again
    want = check(full, full, ONE, domain=dom, connectivity=4, merges=True, tag='cut twice')
    assert want['n_objects'].tolist() == [[4]]


@pytest.mark.parametrize('n_y, n_x', [(65, 67), (257, 259)])
@pytest.mark.parametrize('connectivity, density', [(4, 0.59), (8, 0.41)])
def test_random_fields_at_the_percolation_threshold(n_y, n_x, connectivity, density):
    rng = np.random.default_rng(7 * n_y + connectivity)
    maps = np.stack([field(rng.random((n_y, n_x)) < density, rng) for _ in range(2)])
    obs = field(rng.random((n_y, n_x)) < density, rng)
    for min_area in (1, 2, 5):
        check(maps, obs, ONE, connectivity=connectivity, min_area=min_area, max_objects=8192, merges=True, tag=min_area)


@pytest.mark.parametrize('connectivity, density', [(4, 0.59), (8, 0.41)])
def test_random_field_on_the_largest_grid(connectivity, density):
    rng = np.random.default_rng(connectivity)
    b = rng.random((1023, 1023)) < density
    want = check(field(b, rng), field(b[::-1]), ONE, connectivity=connectivity, min_area=2, max_objects=65535, merges=True, tag='1023')
    assert int(want['area'].max()) > 50000                # (one tortuous cluster spans much of the grid)


def test_table_overflow_true_counts_complete_labels():
    """The 1023 x 1023 checkerboard under 4-connectivity: 523 265 objects, a table of 1000 rows."""
    board = pattern('checkerboard', (1023, 1023))
    want = check(field(board), field(~board), ONE, connectivity=4, max_objects=1000, tag='overflow')
    assert want['n_objects'].tolist() == [[523265]] and want['observed']['n_objects'].tolist() == [523264]
    assert int(want['labels'].max()) == 523265 and want['first'][0, 0, -1] == 2 * 999 and want['first'].shape == (1, 1, 1000)
    # a table one row short, and one that fits exactly
    small = field(pattern('checkerboard', (5, 7)))
    for rows in (17, 18, 19):
        assert check(small, small, ONE, connectivity=4, max_objects=rows, tag=rows)['n_objects'].tolist() == [[18]]


def test_equal_peaks_and_signed_zeros():
    m = np.array([[-0.0, 0.0, -0.0, 0.0, nan, 7.0, 7.0, 1.0, nan, -0.0, -0.0]], f4)
    m = np.concatenate([m, np.full((1, 60), nan, f4), np.array([[2.0, 9.0, 9.0, 9.0, 3.0, 9.0]], f4)], axis=1)     # across a chunk border
    want = check(m, m[:, ::-1].copy(), [-1.0], tag='peaks')
    assert want['peak_cell'][0, 0, :4].tolist() == [1, 5, 9, 72] and want['peak'][0, 0, :4].view(u4).tolist() == [
        0, int(f4(7.0).view(u4)), 0x80000000, int(f4(9.0).view(u4))]
    # the same down a column: the peak comes from another row's wavefront
    check(np.ascontiguousarray(m.T), np.ascontiguousarray(m.T[::-1]), [-1.0], connectivity=8, tag='peaks, column')


def test_no_labels():
    rng = np.random.default_rng(21)
    maps = field(rng.random((2, 33, 70)) < 0.5, rng)
    want = check(maps, maps[1], ONE, labels=False, merges=True, tag='no labels')
    assert 'labels' not in want and 'labels' not in want['observed']


def test_refusals_leave_the_context_usable():
    rng = np.random.default_rng(3)
    maps, obs = field(rng.random((2, 9, 70)) < 0.5, rng), field(rng.random((9, 70)) < 0.5, rng)
    spec = spec_for(9, 70, ONE)
    ctx = context()

    def set_to(name, value):
        def tamper(f):
            o = f.objects.contents
            setattr(o, name, (o.table + 4) if value == 'misaligned' else value)
        return tamper
    for name, value, what in (('connectivity', 6, 'connectivity must be 4 or 8'), ('connectivity', 0, 'connectivity must be 4 or 8'),
                              ('min_area', 0, 'min_area must be at least 1'), ('max_objects', 0, 'max_objects must lie in'),
                              ('max_objects', 65536, 'max_objects must lie in'), ('n_objects', None, 'n_objects or table is NULL'),
                              ('table', None, 'n_objects or table is NULL'), ('table', 'misaligned', 'table must be 8-byte aligned')):
        with pytest.raises(ValueError, match='cpol_objects: ' + what):
            ctx.fractions_maps(maps, obs, spec.fractions, objects=spec, tamper=set_to(name, value))
        check(maps, obs, ONE, merges=True, tag=('after the refusal', what))
    # the labelling scratch above 1 GiB where the summed-area tables pass: 34 sources x 4 thresholds of 1023 x 1023 (refused before
    # anything is uploaded: the maps are pages never touched)
    OB = mods()[1]
    big = spec_for(1023, 1023, FOUR, max_objects=1, labels=False)
    assert OB.scratch_bytes(big, 33) > OB.MAX_SCRATCH_BYTES >= 34 * 4 * 1024 * 1024 * 4
    with pytest.raises(ValueError, match='cpol_objects: the labelling scratch'):
        ctx.fractions_maps(np.zeros((33, 1023, 1023), f4), np.zeros((1023, 1023), f4), big.fractions, objects=big)
    check(maps, obs, ONE, merges=True, tag='after the refused scratch')


def test_without_objects_the_hook_returns_what_it_returned():
    NB, _ = mods()
    rng = np.random.default_rng(5)
    maps, obs = field(rng.random((2, 9, 70)) < 0.5), field(rng.random((9, 70)) < 0.5)
    spec = spec_for(9, 70, ONE)
    got = context().fractions_maps(maps, obs, spec.fractions)
    want = NB.sums(spec.fractions, maps, obs)
    assert isinstance(got, dict) and all(np.array_equal(got[k], want[k]) for k in SUMS)
