"""k_species (cpol_species.inl) alone, through the test hook cpol_debug_read "species_fields", against the NumPy statement of
the rule (cosmo_pol_amd/species.py: fields_of) BIT FOR BIT -- floats compared as their integer views, NaN where the rule has NaN
(the payload of a NaN is not part of the rule).  Rows no sweep produces: absent species, zero columns of either sign,
infinities, negative columns, ties, empty gates, censored gates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_GATES = (1, 63, 64, 65, 257)         # below, at and above a wavefront; more than one workgroup of 256
N_ROWS = (1, 3)
N_HYDRO = (1, 2, 3, 6, 8)
EVERY = ('ZH', 'ZV', 'ZDR', 'KDP', 'RHOHV', 'DELTA_HV', 'ATT_H', 'ATT_V', 'dominant', 'present', 'share', 'sz')
F32 = np.float32


def SP():
    from cosmo_pol_amd import species
    return species


@pytest.fixture(scope='module')
def ctx():
    from cosmo_pol_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def assert_same_bits(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != 'f':
        assert np.array_equal(got, want), what
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, int((np.isnan(got) != nan).sum()))
    a, b = np.ascontiguousarray(got).view(np.uint32)[~nan], np.ascontiguousarray(want).view(np.uint32)[~nan]
    assert np.array_equal(a, b), (what, int((a != b).sum()), a.size)


def chosen_rows(n_rows, n_gates, n_hydro, seed):
    """(sz, zh_final): random rows with a physical leading part (b, cc > 0), and per gate, kind = gate index modulo 12, one of the
    things the kernel can go wrong on."""
    rng = np.random.default_rng(seed)
    sz = rng.uniform(0.05, 2.0, (n_rows, n_gates, n_hydro, 12)).astype(F32)
    sz[..., 0] += F32(5.0)
    sz[..., 3] += F32(5.0)
    sz[..., 4:8] -= F32(1.0)                                   # the phase terms of either sign
    zh = np.ones((n_rows, n_gates), dtype=F32)
    last = n_hydro - 1
    for r in range(n_rows):
        for g in range(n_gates):
            kind = (g + r) % 12
            t = sz[r, g]
            if kind == 1:
                t[rng.integers(n_hydro)] = np.nan              # an absent species
            elif kind == 2:
                t[0] = 0.0                                     # ... written as zeros of either sign
                t[last] = -0.0
            elif kind == 3:
                t[last, 10] = 0.0                              # single zero columns: KDP alone, ATT_V alone
                t[0, 9] = -0.0
            elif kind == 4:
                t[0, rng.integers(12)] = np.inf
                t[last, rng.integers(12)] = -np.inf
            elif kind == 5:
                t[last, :4] = [1.0, 3.0, 3.0, 1.5]             # b < 0: a negative ZH_j, first or last
                t[0, 8:] = -t[0, 8:]
            elif kind == 6:
                t[:] = t[0]                                    # every species ties
            elif kind == 7:
                t[:] = np.nan                                  # an empty gate
            elif kind == 8:
                zh[r, g] = np.nan                              # a censored gate
            elif kind == 9:
                t[last] = t[0]                                 # a tie between the first and the last slot, above the others
                t[0, :4] += F32(20.0)
                t[last, :4] = t[0, :4]
            elif kind == 10:
                t[:, :4] = [1.0, 1.0, 1.0, 1.0]                # b == 0 exactly: ZH_j = 0, ZDR_j = 0, RHOHV_j = x / 0
            elif kind == 11:
                t[0, :4] = F32(3e38)                           # cc overflows
    return sz, zh


def constants():
    return SP().constants_of(0.0533, 0.93)


@pytest.mark.parametrize('n_hydro', N_HYDRO)
@pytest.mark.parametrize('n_rows', N_ROWS)
def test_every_output_equals_the_rule(ctx, n_rows, n_hydro):
    c = constants()
    for n_gates in N_GATES:
        sz, zh = chosen_rows(n_rows, n_gates, n_hydro, 1000 * n_hydro + 10 * n_gates + n_rows)
        want = SP().fields_of(sz, zh, *c)
        got = ctx.species_fields(sz, zh, *c)
        assert set(got) == set(EVERY)
        for k in EVERY[:-1]:
            assert_same_bits(got[k], want[k], (n_rows, n_gates, n_hydro, k))
        assert np.array_equal(got['sz'].view(np.uint32), sz.view(np.uint32)), 'sz'      # (the rows themselves: every bit)
        if n_gates >= 63 and n_hydro >= 2:          # not vacuous: values, empty gates, both kinds of NaN, more than one dominant slot
            assert np.isfinite(want['ZH']).sum() > n_gates and (want['dominant'] == 255).any()
            assert len(set(want['dominant'].ravel()) - {255}) >= 2
            assert (want['ZH'][np.isfinite(want['ZH'])] < 0).any()


@pytest.mark.parametrize('want_only', [('dominant',), ('present',), ('share',), ('KDP',), ('DELTA_HV',), ('RHOHV', 'ZH'), ('sz',),
                                       ('ATT_H', 'dominant', 'present', 'share')])
def test_an_array_left_null_changes_no_other(ctx, want_only):
    c = constants()
    for n_gates, n_hydro in ((65, 3), (257, 6)):
        sz, zh = chosen_rows(3, n_gates, n_hydro, 7 + n_gates)
        want = SP().fields_of(sz, zh, *c)
        want['sz'] = sz
        got = ctx.species_fields(sz, zh, *c, want=want_only)
        assert set(got) == set(want_only)
        for k in want_only:
            assert_same_bits(got[k], want[k], (want_only, k))


def test_refusals_leave_the_context_usable(ctx):
    from cosmo_pol_amd import _native as N
    c = constants()
    sz, zh = chosen_rows(1, 65, 2, 3)
    with pytest.raises(Exception, match='every output pointer is NULL'):
        ctx.species_fields(sz, zh, *c, want=())
    with pytest.raises(ValueError):
        ctx.species_fields(sz[..., :11], zh, *c)
    with pytest.raises(Exception, match='bad shape'):
        ctx.species_fields(np.zeros((1, 4, 9, 12), F32), np.zeros((1, 4), F32), *c)
    got = ctx.species_fields(sz, zh, *c, want=('ZH', 'dominant'))
    want = SP().fields_of(sz, zh, *c)
    assert_same_bits(got['ZH'], want['ZH'])
    assert_same_bits(got['dominant'], want['dominant'])
    assert N.CPOL_MAX_HYDRO == 8
