"""The restatement and the cases of tests/_subsum.py, without a GPU: accumulate() against the oracle's own accumulation, the
coverage of the case list from the columns alone, and the oracle on one case (so that the cases are known to be non-trivial
before they reach a device)."""
import numpy as np
import pytest

import _cases
import _subsum as S
from cosmo_pol_oracle import config as ocfg
from cosmo_pol_oracle import scatter
from cosmo_pol_oracle.beam import nansum_pair


def _oracle_accumulate(terms, present, weights):
    """scatter.radar_observables' accumulation (doppler_scatter.py:124-129, 259-268) on given terms [n_sub, n_gates, 12]:
    nansum_pair sub-beam by sub-beam into a float32 array; per-gate weights divided by their total."""
    n_sub, n_gates, n_col = terms.shape
    sz = np.zeros((n_gates, n_col), dtype='float32') + np.nan
    array_weights = np.ndim(weights) == 2
    if array_weights:
        total = np.sum(np.array([w for w in weights]), axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        for s in range(n_sub):
            valid = present[s]
            if not np.any(valid):
                continue
            if array_weights:
                w = weights[s][valid] / total[valid]
                sz[valid, :] = nansum_pair(sz[valid, :], w[:, None] * terms[s][valid])
            else:
                sz[valid, :] = nansum_pair(sz[valid, :], terms[s][valid] * weights[s])
    return sz


@pytest.mark.parametrize('per_gate', [False, True])
@pytest.mark.parametrize('n_sub', S.COUNTS)
def test_accumulate_is_the_oracles_accumulation(n_sub, per_gate):
    rng = np.random.default_rng(1000 * n_sub + per_gate)
    n_gates = 37
    # terms over twelve decades with both signs, NaNs among them; presence at three densities
    terms = rng.normal(size=(n_sub, n_gates, 12)) * 10.0 ** rng.uniform(-9, 3, (n_sub, n_gates, 1))
    terms[rng.random(terms.shape) < 0.03] = np.nan
    present = rng.random((n_sub, n_gates)) < rng.choice([0.05, 0.5, 1.0], size=n_gates)[None, :]
    if per_gate:
        weights = S.sub_weights(n_sub)[:, None] * (1.0 + 0.2 * rng.random((n_sub, n_gates)))
        weights[rng.random(weights.shape) < 0.1] = 0.0
        weights[0][weights.sum(axis=0) == 0] = 1.0
        present = present & (weights > 0)                  # (the oracle requires quad_weight > 0)
    else:
        weights = S.sub_weights(n_sub)
    got = S.accumulate(terms, present, weights)
    want = _oracle_accumulate(terms, present, weights)
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint32)[~np.isnan(got)], want.view(np.uint32)[~np.isnan(want)])
    assert np.isnan(got[~present.any(axis=0)]).all() and np.isfinite(got).sum() > 12


def test_accumulate_notices_a_swapped_pair():
    """The order is part of the operation: two sub-beams exchanged change bits (what bit equality is for)."""
    rng = np.random.default_rng(5)
    terms = rng.random((9, 200, 12)) + 0.5
    present = np.ones((9, 200), dtype=bool)
    w = S.sub_weights(9)
    a = S.accumulate(terms, present, w)
    swap = [0, 1, 2, 4, 3, 5, 6, 7, 8]
    b = S.accumulate(terms[swap], present, w[swap])
    np.testing.assert_allclose(a, b, rtol=1e-6)
    assert (a != b).sum() > 100


def test_case_list_covers_what_it_must():
    bad = S.coverage_failures()
    assert not bad, '\n'.join(bad)
    for extra in (S.DRY_CASES, S.DOPPLER_CASES):
        for c in extra:
            pres = S.presence(c, S.make_columns(c))
            assert sum(int(p.any()) for p in pres.values()) >= 2, c.name
    assert len(set(c.name for c in S.CASES + S.DRY_CASES + S.DOPPLER_CASES)) == len(S.CASES + S.DRY_CASES + S.DOPPLER_CASES)
    # the weights of any count are distinct and within a factor of 1.4
    for n in S.COUNTS:
        w = S.sub_weights(n)
        assert len(np.unique(w)) == n and w.max() / w.min() <= 1.4


def test_columns_follow_from_the_name_alone():
    c = S.BY_NAME[[k for k in S.BY_NAME if k.startswith('s65_r17_g5_')][0]]
    again = S.Case(c.n_sub, c.n_rays, c.n_gates, c.rot, c.wgate, c.melt)
    a, b = S.make_columns(c), S.make_columns.__wrapped__(again)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert not a[k].flags.writeable


def test_oracle_on_three_rays_of_a_65_subbeam_case():
    case = S.BY_NAME[[k for k in S.BY_NAME if k.startswith('s65_r17_g5_') and 'wgate' not in k][0]]
    cols = S.make_columns(case)
    conf, _, _, _, luts, _ = _cases.radial_case('c4_7x7')
    assert tuple(ocfg.hydrometeor_list(conf)) == S.SPECIES
    ol = {h: _cases.as_oracle_lut(l) for h, l in luts.items()}
    n_finite = n_rvel = 0
    for ray in (0, 8, 16):
        o = scatter.radar_observables(S.oracle_subbeams(case, cols, ray), ol, conf, return_sz=True)
        assert o.sz_integ.shape == (case.n_gates, len(S.SPECIES), 12)
        pres = S.presence(case, cols)
        for j, h in enumerate(S.SPECIES):                  # NaN exactly where the species is absent from every sub-beam
            assert np.array_equal(~np.isnan(o.sz_integ[:, j, 0]), pres[h][ray].any(axis=0)), h
        n_finite += int(np.isfinite(o.sz_integ).sum())
        n_rvel += int(np.isfinite(o.values['RVEL']).sum())
    assert n_finite > 200, n_finite
    assert n_rvel > 3 * case.n_gates / 2, n_rvel
