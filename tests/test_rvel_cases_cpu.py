"""The cases of the radial-velocity pass (tests/_rvel.py) without a GPU: what the cases must stage, and every restatement shown on the
oracle alone (cosmo_pol_oracle.scatter.radar_observables).

  * the coverage of the case list, from the columns; it fails when a listed edge is taken out of the cases;
  * the accumulation: the sequential NaN-skipping definition applied to the oracle's own per-sub-beam terms gives the BITS of the
    oracle's RVEL, with scalar and with per-gate weights;
  * the term: the fall-speed sums the oracle formed (integrate_V, recorded), the ice total at the first VALID gate -- a gate of
    weight 0 is not valid -- and proj_from_moments with NumPy's float32 cosine and sine give the BITS of the oracle's term;
  * k_ice_first's order is a sum of the same numbers: within n 2^-53 of np.sum, the first gate exact, and exactly the plain sum
    where at most one gate is valid;
  * the folding formula is scatter.aliasing;
  * condition (C) of tests/test_gpu_rvel.py: the float64 cosine and sine rounded once to float32 (what the device and the
    restatement form) differ from the np.longdouble value rounded once in at most HALF of the 1e-4 of the gates that the device
    test excepts;
  * condition (F): theta of the reference's RVEL lies farther than 1e-9 from every pole of the tangent at every gate of the
    folding cases -- the condition leaves out no gate;
  * the tolerance of stage (A): the worst relative deviation of the float64 oracle's integrate_V from the same formulas in
    np.longdouble (gamma species: the closed form; ice: the sums over the same float32 diameters and power tables) stays within
    R.ORACLE_WORST = 1.3e-15 (measured: 1.29e-15, graupel of the 1-moment scheme), that of the melting species within
    R.ORACLE_WORST_MELTING = 1.8e-14 (measured: 1.78e-14, melting snow); the device test allows 8 times the figure of the kind."""
import numpy as np
import pytest

import _rvel as R
import _scans
from cosmo_pol_oracle import scatter

CAP_FILE = 1e-4                                          # tests/test_gpu_rvel.py: the share of excepted gates


@pytest.fixture(scope='module')
def oracle():
    kept = {}

    def get(case, ray):
        if (case.name, ray) not in kept:
            kept[(case.name, ray)] = R.oracle_ray(case, ray)
        return kept[(case.name, ray)]
    return get


def test_cases_cover_what_they_claim():
    assert R.coverage_failures() == []
    c = R.CASES[3]
    a, b = R.make_columns(c), R.make_columns(R.Case(c.sset, c.n_gates, n_sub=c.n_sub, n_rays=c.n_rays, rot=c.rot, wgate=c.wgate))
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)          # (from the name alone)


@pytest.mark.parametrize('drop,word', [
    (lambda c: c.wgate, 'first_ice_gate_weight_zero'), (lambda c: c.n_gates == R.N_MAX, 'gate counts'),
    (lambda c: c.n_sub == 29, 'sub-beam counts'), (lambda c: c.sset == 'melt', 'species sets'),
    (lambda c: c.n_sub in (7, 14), 'exact_groups'), (lambda c: c.n_gates > 66, "('first', 64)"),
    (lambda c: c.n_sub > 1, 'mask_drops_one_sub_beam')])
def test_coverage_fails_when_an_edge_is_removed(drop, word):
    bad = R.coverage_failures([c for c in R.CASES if not drop(c)])
    assert any(word in b for b in bad), bad


@pytest.mark.parametrize('case', R.CASES, ids=[c.name for c in R.CASES])
def test_accumulation_is_the_oracles(oracle, case):
    """accumulate() on the oracle's own terms: the bits of the oracle's RVEL.  NaN exactly where no sub-beam has a term."""
    for r in range(case.n_rays):
        o = oracle(case, r)
        want = o['RVEL']
        got = R.accumulate(o['proj'], R.weights_of(case, r))
        assert _scans.same_bits(got, want), (case.name, r, _scans.where_differs(got, want))
        assert np.array_equal(np.isnan(want), np.isnan(o['proj']).all(axis=0)), (case.name, r)


@pytest.mark.parametrize('case', R.CASES, ids=[c.name for c in R.CASES])
def test_term_is_the_oracles(oracle, case):
    """moments() and proj_from_moments() on the sums the oracle's integrate_V returned -- every species at its valid gates, the ice
    total at the FIRST valid gate -- with NumPy's float32 cosine and sine: the bits of the oracle's term."""
    cols = R.make_columns(case)
    pres = R.presence(case)
    sc = R.az_sincos(cols['quad_pts'])
    vsrc = R.vsrc_of(case)
    nh, ng = len(case.species), case.n_gates
    for r in range(case.n_rays):
        o = oracle(case, r)
        for s in range(case.n_sub):
            vn = np.zeros((nh, ng, 2))
            valid = np.stack([pres[h][r, s] for h in case.species])
            first = {j: (R.NO_GATE, 0.0, 0.0) for j in range(nh) if vsrc[j] == 2}
            for h, v, n in o['sums'][s]:
                j = case.species.index(h)
                if vsrc[j] == 2:
                    assert v.shape == (1,) and valid[j].any()
                    first[j] = (int(np.flatnonzero(valid[j])[0]), float(v[0]), float(n[0]))
                else:
                    vn[j, valid[j], 0], vn[j, valid[j], 1] = v, n
            assert {h for h, _, _ in o['sums'][s]} == {h for j, h in enumerate(case.species) if valid[j].any()}
            v, nn = R.moments(vn, valid, vsrc, first)
            got = R.proj_from_moments(v, nn, cols['U'][r, s], cols['V'][r, s], cols['W'][r, s], cols['elev'][r, s], sc[r, s], trig='numpy')
            assert _scans.same_bits(got, o['proj'][s]), (case.name, r, s, _scans.where_differs(got, o['proj'][s]))


def test_ice_total_is_the_sum_over_the_valid_gates():
    """The oracle's one total per sub-beam is the sum of integrate_V restricted to one gate at a time, over the gates that are valid
    (Q > 0 and, with per-gate weights, weight > 0), whatever the order: within n 2^-53 sum|x| -- and the wavefront order is such a sum."""
    n_moved = 0
    for case in (R.BY_NAME['rsgi_g129_s3_r8_p0_wgate'], R.BY_NAME['2mom_g66_s8_r8_p0_wgate'], R.BY_NAME['rsgi_g257_s3_r8_p0']):
        j = case.species.index(R.ICE)
        pres, plain = R.presence(case)[R.ICE], R.presence(case, weights=False)[R.ICE]
        for r in range(case.n_rays):
            o = R.oracle_ray(case, r, subs=[0, 1])
            for s in (0, 1):
                valid = pres[r, s]
                rec = [x for x in o['sums'][s] if x[0] == R.ICE]
                assert bool(rec) == bool(valid.any())
                if not rec:
                    continue
                v, n = R.oracle_moments(case, r, s)
                f, tv, tn = R.ice_first(np.stack([v[j], n[j]], axis=-1), valid)
                assert f == int(np.flatnonzero(valid)[0])
                k = int(valid.sum())
                assert abs(tv - rec[0][1][0]) <= k * 2.0 ** -53 * abs(tv) and abs(tn - rec[0][2][0]) <= k * 2.0 ** -53 * abs(tn)
                # the oracle's term carries the total at that gate and nowhere else: v / n of the other ice gates is unchanged by it
                n_moved += int(plain[r, s].argmax() != f) if plain[r, s].any() else 0
    assert n_moved >= 3                                  # (sub-beams whose first ice gate has weight 0)


def test_wave_order_is_a_sum():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 129, 257, R.N_MAX):
        x = rng.uniform(0.5, 2.0, n)
        for valid in (np.ones(n, dtype=bool), rng.random(n) < 0.5, np.arange(n) == n - 1, np.zeros(n, dtype=bool), np.arange(n) >= 64):
            got = R.wave_sum(x, valid)
            want = float(np.sum(x[valid]))
            assert abs(got - want) <= max(n, 1) * 2.0 ** -53 * abs(want), (n, got, want)
            if valid.sum() <= 1:
                assert got == want
    # the order itself, lane by lane and step by step in plain Python, on 130 gates whose sum depends on the order
    x = rng.uniform(0.5, 2.0, 130) * 10.0 ** rng.uniform(-3, 3, 130)
    lanes = [sum(x[l::64].tolist(), 0.0) for l in range(64)]          # (Python's sum: left to right)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l + off] for l in range(off)]
    assert R.wave_sum(x, np.ones(130, dtype=bool)) == lanes[0]
    assert R.wave_sum(x, np.ones(130, dtype=bool)) != sum(x.tolist(), 0.0)


def test_folding_is_the_oracles():
    rv = np.concatenate([np.linspace(-40.0, 40.0, 2001), [np.nan]])
    for nyq in (0.45, 0.7, 6.0, 11.0):
        assert _scans.same_bits(R.alias(rv, nyq), scatter.aliasing(rv.copy(), nyq))


def test_folding_cases_stay_away_from_the_poles(oracle):
    """Condition (F): no gate of the folding cases is left out."""
    for case in R.ALIAS_CASES:
        nyq = R.nyquist_of(case)
        assert len(np.unique(nyq)) >= 4
        most = 0.0
        for r in range(case.n_rays):
            rv = oracle(case, r)['RVEL']
            ok = ~np.isnan(rv)
            d = R.pole_distance(R.alias_theta(rv[ok], nyq[r]))
            assert (d > R.POLE_MARGIN).all(), (case.name, r, float(d.min()))
            most = max(most, float(np.abs(rv[ok]).max() / nyq[r])) if ok.any() else most
            folded = R.oracle_ray(case, r, nyquist=nyq[r])['RVEL']
            assert _scans.same_bits(folded, R.alias(rv, nyq[r]))
        assert most > 5, (case.name, most)               # several Nyquist intervals


def test_rounded_trig_stays_within_half_the_cap():
    """Condition (C): float32(cos_float64(th)) against float32(cos_longdouble(th)) over every finite gate of the file."""
    n = differ = 0
    for case in R.CASES:
        e = R.fold(np.array(R.make_columns(case)['elev'], dtype=np.float32))
        e = e[~np.isnan(e)]
        ct, st = R.trig32(e)
        ce, se = R.trig32_exact(e)
        n += e.size
        differ += int(((ct != ce) | (st != se)).sum())
    assert n > 20000 and differ <= 0.5 * CAP_FILE * n, (differ, n)


def test_oracle_deviation_from_longdouble_is_what_the_tolerance_says():
    """Stage (A)'s tolerances: measured here, asserted not to exceed R.ORACLE_WORST (gamma species and ice) and
    R.ORACLE_WORST_MELTING (melting snow and graupel: same diameters and PSD parameters, every operation in np.longdouble)."""
    m = {}
    for name in ('rsgi_g65_s7_r8_p1', '2mom_g65_s1_r8_p0', 'rsgi_g129_s3_r8_p0_wgate', '2mom_g129_s8_r8_p2', 'rsg_g129_s1_r6_p0',
                 'rsgi_g257_s3_r8_p0', 'melt_g63_s3_r3_p0', 'melt_g65_s6_r4_p4_wgate'):
        case = R.BY_NAME[name]
        for r in range(case.n_rays):
            for s in range(min(case.n_sub, 3)):
                R.oracle_moments(case, r, s, measure=m)
    print(m)
    assert set(m) == {'R', 'S', 'G', 'H', 'I', 'mS', 'mG'}
    plain, melting = max(v for h, v in m.items() if h not in R.MELTING), max(m[h] for h in R.MELTING)
    assert 0.5 * R.ORACLE_WORST < plain <= R.ORACLE_WORST, m
    assert 0.5 * R.ORACLE_WORST_MELTING < melting <= R.ORACLE_WORST_MELTING, m
    assert R.oracle_rtol('mS') == 8 * R.ORACLE_WORST_MELTING and R.oracle_rtol('I') == R.oracle_rtol('R') == 8 * R.ORACLE_WORST == R.ORACLE_RTOL


def test_melting_sums_take_no_float32_power():
    """tests/_spectrum.py::rounded_powers exists because NumPy's float32 power differs between hosts; the melting species'
    integrate_V on the columns' float64 values takes none: the same bits with and without it."""
    import _spectrum
    case = R.BY_NAME['melt_g63_s3_r3_p0']
    a = R.oracle_moments(case, 0, 0)
    with _spectrum.rounded_powers():
        b = R.oracle_moments(case, 0, 0)
    j = [case.species.index(h) for h in R.MELTING]
    assert np.isfinite(a[0][j]).any() and _scans.same_bits(a[0][j], b[0][j]) and _scans.same_bits(a[1][j], b[1][j])


def test_numpy_trig_accounts_for_the_deviation_from_the_oracle(oracle):
    """What RVEL's deviation from the oracle consists of.  The device forms the float32 cosine and sine as the float64 value rounded
    once; the oracle takes NumPy's float32 functions, which differ from that in the last bit of about one angle in eight.  One unit
    in the last place of a float32 in [0.5, 1] is 2^-24, so a term moves by at most 2^-24 (|U sin(az) + V cos(az)| + |W - vh|): the
    oracle's own terms, re-evaluated with the rounded functions, stay within that, and RVEL formed from them differs from the
    oracle's by at most 1.7e-6 m/s over the file -- the figure the device shows (tests/test_gpu_rvel.py, stage G)."""
    worst = worst_rv = 0.0
    n = differ = 0
    for case in R.CASES:
        cols = R.make_columns(case)
        sc = R.az_sincos(cols['quad_pts'])
        for r in range(case.n_rays):
            o = oracle(case, r)
            terms = []
            for s in range(case.n_sub):
                e = R.fold(np.array(cols['elev'][r, s], dtype=np.float32))
                th = np.deg2rad(e)
                ctn, stn = np.cos(th), np.sin(th)
                ct, st = R.trig32(e)
                U, V = (cols[k][r, s].astype(np.float64) for k in 'UV')
                hor = U * sc[r, s, 0] + V * sc[r, s, 1]
                with np.errstate(invalid='ignore', divide='ignore'):
                    fall = (o['proj'][s] - hor * ctn.astype(np.float64)) / stn.astype(np.float64)         # W - vh of the oracle's term
                    alt = hor * ct.astype(np.float64) + fall * st.astype(np.float64)
                    d = np.abs(alt - o['proj'][s])
                    bound = 2.0 ** -24 * (np.abs(hor) + np.abs(fall)) + 1e-12
                ok = np.isfinite(d)
                assert (d[ok] <= bound[ok]).all(), (case.name, r, s)
                worst = max(worst, float(d[ok].max())) if ok.any() else worst
                n += int(ok.sum())
                differ += int(((ctn != ct) | (stn != st))[ok].sum())
                terms.append(alt)
            d = np.abs(R.accumulate(np.array(terms), R.weights_of(case, r)) - o['RVEL'])
            if np.isfinite(d).any():
                worst_rv = max(worst_rv, float(np.nanmax(d)))
    print(dict(worst_term=worst, worst_rvel=worst_rv, terms=n, terms_with_another_cosine_or_sine=differ))
    assert 0 < worst_rv <= 1e-5 and worst_rv <= R.ATOL / 20 and differ > 0.01 * n
