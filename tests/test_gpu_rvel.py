"""The radial velocity of Doppler scheme 1 -- k_classify's analytic moments, k_ice_first, subbeam_proj / proj_from_moments,
k_rvel_terms, the accumulation and the folding of gate_finish (cosmo_pol_amd/csrc/cpol_final.inl) -- at every gate count,
sub-beam count and species set of tests/_rvel.py, through RadarOperator.simulate_columns.

The stages are separated with three read-only debug buffers (item_vn, item_vmask, ice_first):
  (A) moments: item_vn of the gamma species against integrate_V's closed form in np.longdouble from the device's own lambda and N0
      (item_par rows 0 and 1) within 2e-15 (1 + |p ln lambda|) + 8 2^-53 (derived at gamma_bound); the 2-moment n is the float32 QN
      exactly; the sums of every gamma species and of ice (bin by bin, CPOL_ITAB=0) against the oracle's own integrate_V within
      _rvel.ORACLE_RTOL -- 8 times the oracle's own distance from np.longdouble, measured in tests/test_rvel_cases_cpu.py; the
      table-borne sums of ice and the melting species against the bin-by-bin run within what itab_check reports for the slot;
      the melting species' bin-by-bin sums against the oracle within 8 times ITS distance from np.longdouble (1.8e-14: the
      finite difference in get_N).  In the columns' float64 evaluation the oracle's melting PSD takes no float32 power
      (tests/_spectrum.py::rounded_powers changes none of its bits here: asserted on the CPU).  The oracle comparison runs on 8
      of the 24 cases and the first three sub-beams of every ray;
  (B) k_ice_first: ice_first.v and .n are the BITS of the wavefront order (_rvel.wave_sum) applied to the run's own item_vn, the
      first gate exact, 0x7fffffff where a sub-beam has no valid ice;
  (C) the term: every sub-beam alone with weight 1.0 and no folding gives RVEL = 0 + proj 1.0 / 1.0 = proj, which must be the BITS
      of the restated subbeam_proj on item_vn, ice_first and the columns; a gate is excepted only where moving the float32 cosine
      or sine by one ulp accounts for it, at most 1e-4 of the file's finite gates;
  (D) the accumulation: RVEL of every multi-sub-beam case is the BITS of the sequential definition (_rvel.accumulate) on the alone
      terms of (C) and the weights (sub_w[s], or the per-gate weights): k_rvel_terms, the groups of seven, the tail, and the
      in-place form below four sub-beams; NaN exactly where the oracle's RVEL is NaN;
  (E) launch forms: the same bits with the debug reads off, CPOL_SUBSUM=0, every k_subbeam_sum form, and for one sub-beam
      CPOL_GATE1 0 / 1 / 2, CPOL_GATE1_SPECIES 0 / 2, CPOL_GATE1_RAY 0 / 1 / 2, each form asserted from launch_forms() as far as
      it records them; which k_subbeam_sum form, k_gate1_species, k_rvel_terms and k_final width a knob set selects is asserted
      on the host through choose_forms for this file's FORM_PLAN (tests/test_forms_cpu.py);
  (F) the folding: against the restated formula on the unfolded run within 16 2^-53 (|rv| + nyq), |out| <= nyq (1 + 2^-50), NaN kept;
  (G) end to end: every case against the oracle at the suite's 2e-4 m/s.
The worst deviation of every stage is printed as a JSON line and, when CPOL_PARITY_DIR names a directory, appended to
rvel_parity_records.jsonl there (profiles/ keeps a copy).

Measured on the library as it is (188 tests, all pass): (A) the closed form within 0.17 of its bound on 127 000 items, the oracle
within 7.7e-15 (allowed 1.04e-14; melting snow 3.6e-14 and melting graupel 2.0e-14 of 1.44e-13), the tables within 7.9e-14 of 8.4e-14 (ice) and 4.5e-15 of 7.5e-12 (melting snow); (B) 678
records, 94 without ice, up to 4 906 valid gates: the bits; (C) 53 764 terms: the bits, none excepted; (D) 18 cases: the bits;
(F) within 0.16 of the bound, up to 51 Nyquist intervals; (G) 1.7e-6 m/s at worst on 16 783 gates -- NumPy's float32 cosine and
sine against the rounded ones, as tests/test_rvel_cases_cpu.py shows on the host alone.

Tried against scratch builds of the library with one edit each, every index kept inside its buffer (the child-process test left
out: it loads the installed library):
  * k_ice_first without the strided continuation (`g < n_gates && g < 64`): 30 fail --
    test_ice_first_carries_the_bits_of_the_wavefront_order in all 15 cases with ice beyond 64 gates (65 gates included; the 1-,
    2-, 17-, 33-, 63- and 64-gate cases pass, as they must) and test_rvel_meets_the_oracle in the same 15: the total is credited
    to ONE gate per (ray, sub-beam), which then misses 2e-4 m/s by far.  (C), (D) and (E) pass: they restate from the run's own
    ice_first.
  * the tree's last step dropped (`off >= 2`): 37 fail -- (B) in 19 of the 21 cases with ice (the 1-gate case has nothing in
    lane 1; at 17 gates the planned ice sits in lane 16 alone) and (G) in 18.
  * `first` not reduced over the lanes: 38 fail -- (B) and (G) in 19 cases each: first_gate is wrong wherever the first valid ice
    gate is not gate 0, 64, 128 ... (lane 0's own gates).
  * the batch loop's tail skipped (`s < a.n_sub && !a.proj`): 27 fail -- test_accumulation_carries_the_bits_of_the_definition in
    the 9 cases whose sub-beam count from 4 on is no multiple of 7 (4, 6, 8, 13, 15, 22, 29 and the per-gate cases of 6 and 8;
    7 and 14 pass, as do 2 and 3: in place), (G) in the same 9, and the 9 launch forms of the 6-sub-beam case (every RVEL NaN).
  * `tw` counting NaN terms: 65 fail -- test_term_carries_the_bits_of_subbeam_proj in 22 of 24 cases (a sub-beam alone whose term
    is NaN must give NaN, not 0 / 1), (D) in 17 of 18, (G) in 22 of 24, (F) in 3 of 4.
  * reflect_index applied once: tests/test_gpu_ml_weights.py (see there)."""
import json
import os

import numpy as np
import pytest

import _cases
import _rvel as R
import _scans

pytestmark = pytest.mark.gpu

KNOBS = ('CPOL_GATE1', 'CPOL_GATE1_RAY', 'CPOL_GATE1_SPECIES', 'CPOL_FUSE_GATE1', 'CPOL_FUSE_CLASSIFY', 'CPOL_RARE_DIRECT', 'CPOL_SUBSUM',
         'CPOL_SUBSUM_TEAM', 'CPOL_SUBSUM_COOP', 'CPOL_SUBSUM_FORM', 'CPOL_SUBSUM_SMALL', 'CPOL_SUBSUM_CHAIN', 'CPOL_FINAL_512',
         'CPOL_USE_GRAPH', 'CPOL_EXP_SKIP', 'CPOL_ITAB', 'CPOL_ITAB_MELT')
ICE_REC = np.dtype([('first_gate', '<i4'), ('pad', '<i4'), ('v', '<f8'), ('n', '<f8')])
CAP_FILE = 1e-4                                          # (C): gates excepted by the one-ulp rule, share of the file's finite gates
# (A) the closed form v = c lambda^p on the device: cp_exp(p cp_log(lambda)) with cp_log and cp_exp each within 2e-15 relative
# (tests/test_gpu_math.py).  The logarithm's error 2e-15 |ln lambda| is multiplied by |p| in the exponent and becomes a relative
# error 2e-15 |p ln lambda| of the power; cp_exp adds its own 2e-15; the product p ln lambda, the three factors in front and the
# division by nu are six float64 roundings, a seventh for the exponent's own rounding scaled like the first term (inside it),
# bounded together by 8 2^-53.  Hence 2e-15 (1 + |p ln lambda|) + 8 2^-53.
MATH_RTOL = 2e-15


def gamma_bound(p, lam):
    return MATH_RTOL * (1.0 + np.abs(p * np.log(lam))) + 8 * 2.0 ** -53


def _ids(cases):
    return [c.name for c in cases]


def _record(**kw):
    print(json.dumps(kw))
    out = os.environ.get('CPOL_PARITY_DIR')
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'rvel_parity_records.jsonl'), 'a') as f:
        f.write(json.dumps(kw) + '\n')


class Runs(object):
    """One operator per (species set, knobs, Nyquist file); every run is kept."""

    def __init__(self):
        self.ops, self.kept, self.book = {}, {}, {}

    def operator(self, sset, knobs=(), nyquist_file=None):
        key = (sset, tuple(knobs), nyquist_file)
        if key not in self.ops:
            from cosmo_pol_amd import RadarOperator
            conf = R.oracle_setup(sset)[0]
            luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in R.oracle_setup(sset)[2]}
            with pytest.MonkeyPatch.context() as mp:
                for k in KNOBS:
                    mp.delenv(k, raising=False)
                for k, v in knobs:
                    mp.setenv(k, str(v))
                self.ops[key] = RadarOperator(config=R.config_overrides(sset, nyquist_file), luts=luts, output_variables='only_radar')
            got = self.ops[key].config
            assert got['doppler']['scheme'] == 1 and got['radar']['radial_resolution'] == R.RADIAL_RES, got
            assert (got['radar']['nyquist_velocity'] is not None) == (nyquist_file is not None)
        return self.ops[key]

    def run(self, case, sub=None, debug=True, knobs=(), nyquist_file=None, keep=True, diagnose=False):
        """-> dict(RVEL [n_rays, n_gates], forms, and with debug: vn [n_hydro, n_rays, n_sub, n_gates, 2], valid [n_hydro, n_rays,
        n_sub, n_gates], ice (records [n_rays, n_sub]; None without ice), par [n_hydro, 6, n_rays, n_sub, n_gates]).  sub: that
        sub-beam alone (R.alone); None: the case as it is.  diagnose: without the given melting fields -- the device diagnoses the
        melting layer from QR, QS and QG itself (the single-beam kernels take no given fields)."""
        key = (case.name, sub, debug, tuple(knobs), nyquist_file, diagnose)
        if key in self.kept and keep:                    # (keep False: always a fresh run)
            return self.kept[key]
        op = self.operator(case.sset, knobs, nyquist_file)
        cols = dict(R.make_columns(case)) if sub is None else R.alone(case, sub)
        if diagnose:
            cols = {k: v for k, v in cols.items() if k not in ('QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG', 'has_melting')}
        n_sub = case.n_sub if sub is None else 1
        ctx = op._lane(0)
        ctx.enable_debug(bool(debug))
        res = op.simulate_columns(cols)
        assert res['n_sub'] == n_sub and res['RVEL'].shape == (case.n_rays, case.n_gates) and res['RVEL'].dtype == np.float64
        forms = ctx.launch_forms()
        assert forms['n_sub'] == n_sub, forms
        out = {'RVEL': res['RVEL'], 'forms': forms}
        if debug and not diagnose:
            assert forms['gate1'] == 0, forms
            nh, shape = len(case.species), (case.n_rays, n_sub, case.n_gates)
            n_sbg = int(np.prod(shape))
            out['vn'] = ctx.debug_read('item_vn', (nh, n_sbg, 2), np.float64).reshape((nh,) + shape + (2,))
            bits = ctx.debug_read('item_vmask', (n_sbg,), np.uint8).reshape(shape)
            out['valid'] = np.stack([(bits >> j) & 1 == 1 for j in range(nh)])
            out['par'] = ctx.debug_read('item_par', (nh, 6, n_sbg), np.float64).reshape((nh, 6) + shape)
            out['ice'] = ctx.debug_read('ice_first', (case.n_rays, n_sub), ICE_REC) if case.has_ice() else None
            ctx.enable_debug(False)
        if keep:
            self.kept[key] = out
        return out

    def close(self):
        for op in self.ops.values():
            op.close()
        self.ops = {}


@pytest.fixture(scope='module')
def runs():
    r = Runs()
    yield r
    r.close()


@pytest.fixture(scope='module')
def oracle():
    """(case, ray) -> R.oracle_ray of the case as it is, computed once."""
    kept = {}

    def get(case, ray):
        if (case.name, ray) not in kept:
            kept[(case.name, ray)] = R.oracle_ray(case, ray)
        return kept[(case.name, ray)]
    return get


def _valid_is_the_columns(case, out, sub=None):
    pres = R.presence(case)
    for j, h in enumerate(case.species):
        want = pres[h] if sub is None else pres[h][:, sub:sub + 1]
        assert np.array_equal(out['valid'][j], want), (case.name, sub, h)


# ------------------------------------------------------------------------------------------------------------------ (A) moments
@pytest.mark.parametrize('case', R.CASES, ids=_ids(R.CASES))
def test_analytic_moments_are_the_closed_form(runs, case):
    """(A), the gamma species: item_vn against integrate_V's closed form (hydrometeors.py:178-199) in np.longdouble from the
    device's own lambda and N0."""
    from cosmo_pol_oracle.psd import create_hydrometeor
    out = runs.run(case)
    _valid_is_the_columns(case, out)
    scheme = R.oracle_setup(case.sset)[0]['microphysics']['scheme']
    cols = R.make_columns(case)
    worst_v = worst_n = 0.0
    n_items = 0
    L = np.longdouble
    for j, h in enumerate(case.species):
        if h == R.ICE or h in R.MELTING:
            continue
        hyd = create_hydrometeor(h, scheme)
        ok = out['valid'][j]
        if not ok.any():
            continue
        lam, n0 = out['par'][j, 0][ok], out['par'][j, 1][ok]
        if scheme == '1mom' and h in ('R', 'G'):
            n0 = np.full_like(lam, float(hyd.N0))        # (the fixed intercept: the parameter slot is not used)
        v, n = out['vn'][j][ok][:, 0], out['vn'][j][ok][:, 1]
        assert np.isfinite(lam).all() and (lam > 0).all() and np.isfinite(v).all() and np.isfinite(n).all(), (case.name, h)
        pv = -(hyd.beta + hyd.mu + 1) / hyd.nu
        want_v = L(hyd.vel_factor) * L(n0) * L(hyd.alpha) / L(hyd.nu) * np.exp(L(pv) * np.log(L(lam)))
        rel = np.abs((L(v) - want_v) / want_v).astype(np.float64)
        assert (rel <= gamma_bound(pv, lam)).all(), (case.name, h, 'v', float((rel / gamma_bound(pv, lam)).max()))
        worst_v = max(worst_v, float((rel / gamma_bound(pv, lam)).max()))
        if scheme == '2mom':
            qn = cols['QN' + h + '_v'][ok]
            assert qn.dtype == np.float32 and np.array_equal(n, qn.astype(np.float64)), (case.name, h)
        else:
            pn = -(hyd.mu + 1) / hyd.nu
            want_n = L(hyd.ntot_factor) * L(n0) / L(hyd.nu) * np.exp(L(pn) * np.log(L(lam)))
            rel = np.abs((L(n) - want_n) / want_n).astype(np.float64)
            assert (rel <= gamma_bound(pn, lam)).all(), (case.name, h, 'n', float((rel / gamma_bound(pn, lam)).max()))
            worst_n = max(worst_n, float((rel / gamma_bound(pn, lam)).max()))
        n_items += int(ok.sum())
    _record(stage='A_closed_form', case=case.name, items=n_items, worst_share_of_bound_v=worst_v, worst_share_of_bound_n=worst_n)
    assert n_items > 0


# (8 of the 24 cases, every species set among them, and the first three sub-beams of every ray: the oracle, item by item, is slow)
ORACLE_CASES = [R.BY_NAME[k] for k in ('rsgi_g65_s7_r8_p1', '2mom_g65_s1_r8_p0', 'rsgi_g129_s3_r8_p0_wgate', '2mom_g129_s8_r8_p2',
                                         'rsg_g129_s1_r6_p0', 'rsgi_g257_s3_r8_p0', 'melt_g63_s3_r3_p0', 'melt_g65_s6_r4_p4_wgate')]
NO_TABLES = (('CPOL_ITAB', 0),)


@pytest.mark.parametrize('case', ORACLE_CASES, ids=_ids(ORACLE_CASES))
def test_moments_meet_the_oracles_own_evaluation(runs, case):
    """(A), every species: the per-item v and n against the oracle's integrate_V (ice: restricted to one gate); the sums of ice and
    of the melting species bin by bin (CPOL_ITAB=0).  The tolerance is R.oracle_rtol(species): 8 times the worst deviation of the
    float64 oracle from the same formulas in np.longdouble (tests/test_rvel_cases_cpu.py measures it), 1.04e-14 for the gamma
    species and ice, 1.44e-13 for the melting species."""
    out = runs.run(case)
    binned = case.has_ice() or case.melt
    plain = runs.run(case, knobs=NO_TABLES) if binned else out
    if binned:
        off = runs.operator(case.sset, NO_TABLES)._ctx.itab_report()
        assert (off['check'][:len(case.species)] == 0).all()               # (no slot on a table)
    worst = {}
    for r in range(case.n_rays):
        for s in range(min(case.n_sub, 3)):
            v, n = R.oracle_moments(case, r, s)
            for j, h in enumerate(case.species):
                ok = out['valid'][j, r, s]
                assert np.array_equal(ok, ~np.isnan(v[j])), (case.name, r, s, h)
                if not ok.any():
                    continue
                got = (plain if h == R.ICE or h in R.MELTING else out)['vn'][j, r, s][ok]
                dev = max(float(np.abs(got[:, 0] / v[j][ok] - 1).max()), float(np.abs(got[:, 1] / n[j][ok] - 1).max()))
                worst[h] = max(worst.get(h, 0.0), dev)
    _record(stage='A_oracle', case=case.name, tolerance={h: R.oracle_rtol(h) for h in worst}, **{'worst_' + h: x for h, x in worst.items()})
    assert set(worst) == set(case.species), worst
    assert all(x <= R.oracle_rtol(h) for h, x in worst.items()), worst


TABLE_CASES = [R.BY_NAME[k] for k in ('rsgi_g65_s7_r8_p1', '2mom_g65_s1_r8_p0', 'melt_g63_s3_r3_p0', 'melt_g257_s1_r8_p0', 'rsgi_g257_s3_r8_p0')]


@pytest.mark.parametrize('case', TABLE_CASES, ids=_ids(TABLE_CASES))
def test_table_borne_sums_stay_within_the_staging_check(runs, case):
    """(A), the sums that come from an integral table (ice crystals, melting snow and graupel): the table run against the bin-by-bin
    run of the same library (CPOL_ITAB=0), bounded by the accuracy the staging itself reports for the slot (itab_check: the worst
    |polynomial - integrating kernel| / scale over its check points, scale >= the value itself) -- here relative to the bin-by-bin
    value, which is no looser.  The gamma species' analytic moments do not depend on the tables: the same bits."""
    tab, plain = runs.run(case), runs.run(case, knobs=NO_TABLES)
    rep = runs.operator(case.sset)._ctx.itab_report()
    off = runs.operator(case.sset, NO_TABLES)._ctx.itab_report()
    worst = {}
    for j, h in enumerate(case.species):
        ok = tab['valid'][j]
        assert np.array_equal(ok, plain['valid'][j])
        if not ok.any():
            continue
        a, b = tab['vn'][j][ok], plain['vn'][j][ok]
        assert off['check'][j] == 0, (h, off['check'][j])
        if h != R.ICE and h not in R.MELTING:
            assert _scans.same_bits(a, b), (case.name, h)
            continue
        bound = max(float(rep['check'][j]), float(rep['check_edge'][j]))
        assert 0 < bound < 1e-10, (case.name, h, bound)  # (an accepted table)
        dev = float((np.abs(a - b) / np.abs(b)).max())
        worst[h] = (dev, bound)
    _record(stage='A_tables', case=case.name, **{h: {'worst_rel': d, 'itab_check': b} for h, (d, b) in worst.items()})
    assert worst and all(0 < d <= b for d, b in worst.values()), worst


def test_incomplete_buffers_are_refused(runs):
    """item_vn, item_vmask and ice_first are read back only where the last sweep wrote them completely: not after the single-beam
    kernels (the moments stay in registers), ice_first not without a species whose sums are totals over the ray -- a ValueError
    that says so, and the context goes on."""
    case = R.BY_NAME['rsg_g129_s1_r6_p0']
    base = runs.run(case, keep=False)                    # (a fresh run: this context's last sweep)
    ctx = runs.operator(case.sset)._lane(0)
    n_sbg = case.n_rays * case.n_gates
    with pytest.raises(ValueError, match='ice_first is not written'):
        ctx.debug_read('ice_first', (case.n_rays, 1), ICE_REC)
    assert ctx.debug_read('item_vmask', (n_sbg,), np.uint8).any()          # (the general sequence of the debug run: still readable)
    fast = runs.run(case, debug=False, keep=False)
    assert fast['forms']['gate1'] == 1
    for name, shape, dtype in (('item_vn', (len(case.species), n_sbg, 2), np.float64), ('item_vmask', (n_sbg,), np.uint8)):
        with pytest.raises(ValueError, match=name + ' is incomplete'):
            ctx.debug_read(name, shape, dtype)
    assert _scans.same_bits(runs.run(case, keep=False)['RVEL'], base['RVEL'])


# ----------------------------------------------------------------------------------------------------------------- (B) k_ice_first
ICE_CASES = [c for c in R.CASES if c.has_ice()]


@pytest.mark.parametrize('case', ICE_CASES, ids=_ids(ICE_CASES))
def test_ice_first_carries_the_bits_of_the_wavefront_order(runs, case):
    """(B).  A lost chunk beyond gate 64, a dropped step of the tree or an unreduced first gate moves one record."""
    out = runs.run(case)
    _valid_is_the_columns(case, out)
    j = case.species.index(R.ICE)
    first_want, count = R.first_ice_gates(case)
    n_none = 0
    for r in range(case.n_rays):
        for s in range(case.n_sub):
            rec = out['ice'][r, s]
            f, v, n = R.ice_first(out['vn'][j, r, s], out['valid'][j, r, s])
            assert int(rec['first_gate']) == f == int(first_want[r, s]), (case.name, r, s, int(rec['first_gate']), f)
            assert _scans.same_bits(np.array([rec['v'], rec['n']]), np.array([v, n])), (case.name, r, s, case.ice_kind(r), rec, v, n)
            if f == R.NO_GATE:
                n_none += 1
                assert rec['v'] == 0.0 and rec['n'] == 0.0
            else:
                assert rec['v'] > 0 and rec['n'] > 0
    _record(stage='B_ice_first', case=case.name, records=case.n_rays * case.n_sub, without_ice=n_none,
            most_valid_gates=int(count.max()))


# --------------------------------------------------------------------------------------------------------------------- (C) the term
def _term_stage(runs, case):
    """Every sub-beam of the case alone: -> dict(terms [n_sub, n_rays, n_gates] the alone runs' RVEL, finite, excepted, failed)."""
    if case.name in runs.book:
        return runs.book[case.name]
    cols = R.make_columns(case)
    vsrc = R.vsrc_of(case)
    tot = dict(case=case.name, finite=0, excepted=0, failed=0, first=None)
    terms = np.empty((case.n_sub, case.n_rays, case.n_gates))
    for sub in range(case.n_sub):
        out = runs.run(case, sub=sub)
        _valid_is_the_columns(case, out, sub)
        got = out['RVEL']
        terms[sub] = got
        sc = R.az_sincos(cols['quad_pts'])
        for r in range(case.n_rays):
            first = None
            if case.has_ice():
                rec = out['ice'][r, 0]
                first = {case.species.index(R.ICE): (int(rec['first_gate']), float(rec['v']), float(rec['n']))}
            v, nn = R.moments(out['vn'][:, r, 0], out['valid'][:, r, 0], vsrc, first)
            args = (v, nn, cols['U'][r, sub], cols['V'][r, sub], cols['W'][r, sub], cols['elev'][r, sub], sc[r, sub])
            want = R.proj_from_moments(*args)
            if case.wgate:                               # (a gate of weight 0: 0 / 0)
                want = np.where(cols['quad_weights'][r, sub] > 0, want, np.nan)
            assert np.array_equal(np.isnan(got[r]), np.isnan(want)), (case.name, sub, r, _scans.where_differs(got[r], want))
            differ = ~np.isnan(want) & (got[r] != want)
            tot['finite'] += int((~np.isnan(want)).sum())
            if differ.any():
                # the one-ulp rule: the float32 cosine or sine moved by one unit in its last place accounts for the gate
                settled = np.zeros_like(differ)
                for nudge in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
                    settled |= differ & (R.proj_from_moments(*args, nudge=nudge) == got[r])
                tot['excepted'] += int((differ & settled).sum())
                tot['failed'] += int((differ & ~settled).sum())
                if (differ & ~settled).any() and tot['first'] is None:
                    g = int(np.flatnonzero(differ & ~settled)[0])
                    tot['first'] = (sub, r, g, float(got[r, g]), float(want[g]))
    tot['terms'] = terms
    runs.book[case.name] = tot
    return tot


@pytest.mark.parametrize('case', R.CASES, ids=_ids(R.CASES))
def test_term_carries_the_bits_of_subbeam_proj(runs, case):
    """(C)."""
    t = _term_stage(runs, case)
    _record(stage='C_term', **{k: v for k, v in t.items() if k != 'terms'})
    assert t['failed'] == 0, {k: v for k, v in t.items() if k != 'terms'}
    assert t['finite'] > 0


def test_term_excepted_gates_of_the_file(runs):
    tot = dict(finite=0, excepted=0)
    for case in R.CASES:
        t = _term_stage(runs, case)
        tot['finite'] += t['finite']
        tot['excepted'] += t['excepted']
    _record(stage='C_term', case='the file', **tot)
    assert tot['finite'] > 20000 and tot['excepted'] <= CAP_FILE * tot['finite'], tot


# ----------------------------------------------------------------------------------------------------------- (D) the accumulation
@pytest.mark.parametrize('case', R.MULTI, ids=_ids(R.MULTI))
def test_accumulation_carries_the_bits_of_the_definition(runs, oracle, case):
    """(D).  k_rvel_terms and the groups of seven plus the tail from 4 sub-beams on, the in-place form below."""
    terms = _term_stage(runs, case)['terms']
    multi = runs.run(case)
    assert multi['forms']['gate1'] == 0
    worst = 0.0
    for r in range(case.n_rays):
        want = R.accumulate(terms[:, r], R.weights_of(case, r))
        got = multi['RVEL'][r]
        assert _scans.same_bits(got, want), '%s ray %d (%s, %s): %s' % (case.name, r, case.ice_kind(r), case.drop_kind(r), _scans.where_differs(got, want))
        o = oracle(case, r)['RVEL']
        assert np.array_equal(np.isnan(got), np.isnan(o)), (case.name, r)
        if (~np.isnan(o)).any():
            worst = max(worst, float(np.nanmax(np.abs(got - o))))
    _record(stage='D_accumulation', case=case.name, n_sub=case.n_sub, worst_abs_vs_oracle=worst)


# -------------------------------------------------------------------------------------------------------------------- (G) end to end
@pytest.mark.parametrize('case', R.CASES, ids=_ids(R.CASES))
def test_rvel_meets_the_oracle(runs, oracle, case):
    """(G): the suite's 2e-4 m/s, and how the deviation splits: the oracle's terms against the device's (the moments and NumPy's
    float32 cosine and sine), nothing from the accumulation (D)."""
    got = runs.run(case)['RVEL']
    worst, worst_rel, n = 0.0, 0.0, 0
    for r in range(case.n_rays):
        o = oracle(case, r)['RVEL']
        assert np.array_equal(np.isnan(got[r]), np.isnan(o)), (case.name, r, _scans.where_differs(got[r], o))
        ok = ~np.isnan(o)
        if ok.any():
            err = np.abs(got[r][ok] - o[ok])
            worst = max(worst, float(err.max()))
            worst_rel = max(worst_rel, float((err / np.maximum(np.abs(o[ok]), 1e-300)).max()))
            n += int(ok.sum())
    _record(stage='G_end_to_end', case=case.name, gates=n, worst_abs_RVEL=worst, worst_rel_RVEL=worst_rel)
    assert worst <= R.ATOL, worst
    assert n > 0


# ------------------------------------------------------------------------------------------------------------- (E) launch forms
def _knobs(**kw):
    return tuple(sorted(kw.items()))


SUM_FORMS = {'gather': _knobs(CPOL_SUBSUM_TEAM=0, CPOL_SUBSUM_COOP=0), 'lds': _knobs(CPOL_SUBSUM_TEAM=0, CPOL_SUBSUM_COOP=1),
             'scalar': _knobs(CPOL_SUBSUM_TEAM=0, CPOL_SUBSUM_COOP=1, CPOL_SUBSUM_FORM='scalar'),
             'small': _knobs(CPOL_SUBSUM_TEAM=0, CPOL_SUBSUM_COOP=0, CPOL_SUBSUM_SMALL=1), 'team2': _knobs(CPOL_SUBSUM_TEAM=2),
             'team3_barrier': _knobs(CPOL_SUBSUM_TEAM=3, CPOL_SUBSUM_CHAIN=0), 'team8': _knobs(CPOL_SUBSUM_TEAM=8)}
# case -> the knob sets it is eligible for beyond the default, each with the launch forms it must reach
MANY = {'subbeam_sum': 1, 'gate1': 0, 'final_inplace': 0}
PLAIN = {'subbeam_sum': 0, 'gate1': 0, 'final_inplace': 0}
FORM_PLAN = []
for _name in ('rsgi_g65_s7_r8_p1', 'rsgi_g70_s14_r5_p1_wgate', 'melt_g65_s6_r4_p4_wgate'):
    FORM_PLAN += [(_name, 'default', (), MANY), (_name, 'subsum0', _knobs(CPOL_SUBSUM=0), PLAIN)]
    FORM_PLAN += [(_name, k, v, MANY) for k, v in SUM_FORMS.items()]
for _name in ('2mom_g129_s8_r8_p2', 'melt_g17_s15_r3_p2', 'rsg_g65_s13_r3_p0'):
    FORM_PLAN += [(_name, 'default', (), MANY), (_name, 'subsum0', _knobs(CPOL_SUBSUM=0), PLAIN), (_name, 'team2', SUM_FORMS['team2'], MANY)]
# fewer than four sub-beams: the table items evaluated inside k_final where no table carries Doppler sums, stored otherwise
FORM_PLAN += [('rsg_g130_s3_r3_p1', 'default', (), {'final_inplace': 1, 'subbeam_sum': 0, 'gate1': 0}),
              ('rsg_g130_s3_r3_p1', 'subsum0', _knobs(CPOL_SUBSUM=0), PLAIN),
              ('rsgi_g257_s3_r8_p0', 'default', (), PLAIN), ('rsgi_g257_s3_r8_p0', 'subsum0', _knobs(CPOL_SUBSUM=0), PLAIN),
              ('melt_g127_s2_r4_p1', 'default', (), PLAIN)]
# one sub-beam: the single-beam kernels.  Without ice k_gate1_ray takes the moments from its registers (`have_moments`); with ice
# k_gate1 stores every item (`store_items`) and k_final recomputes the gate that receives the total (`ice_redo`)
G1 = {'gate1': 1, 'gate1_ray': 0}
G1R = {'gate1': 1, 'gate1_ray': 1}
G0 = {'gate1': 0, 'gate1_ray': 0}
FORM_PLAN += [('rsg_g129_s1_r6_p0', 'default', (), G1), ('rsg_g129_s1_r6_p0', 'gate1_0', _knobs(CPOL_GATE1=0), G0),
              ('rsg_g129_s1_r6_p0', 'species0', _knobs(CPOL_GATE1_SPECIES=0), G1), ('rsg_g129_s1_r6_p0', 'species2', _knobs(CPOL_GATE1_SPECIES=2), G1),
              ('rsg_g129_s1_r6_p0', 'ray0', _knobs(CPOL_GATE1_RAY=0), G1), ('rsg_g129_s1_r6_p0', 'ray1', _knobs(CPOL_GATE1_RAY=1), G1R),
              ('rsg_g129_s1_r6_p0', 'ray2', _knobs(CPOL_GATE1_RAY=2), G1R),
              ('rsgi_g129_s1_r14_p5', 'default', (), G1), ('rsgi_g129_s1_r14_p5', 'gate1_0', _knobs(CPOL_GATE1=0), G0),
              ('rsgi_g129_s1_r14_p5', 'ray1', _knobs(CPOL_GATE1_RAY=1), G1),
              ('rsgi_g1_s1_r8_p0', 'default', (), G1), ('rsgi_g5460_s1_r1_p2', 'default', (), G1),
              ('2mom_g65_s1_r8_p0', 'default', (), G1), ('2mom_g65_s1_r8_p0', 'gate1_0', _knobs(CPOL_GATE1=0), G0),
              ('melt_g257_s1_r8_p0', 'default', (), G0)]


@pytest.mark.parametrize('name,form,knobs,want', FORM_PLAN, ids=['%s-%s' % (a, b) for a, b, _, _ in FORM_PLAN])
def test_launch_forms_give_the_same_bits(runs, name, form, knobs, want):
    """(E): the debug reads off, under the knobs of `form`: RVEL is the bits of the general sequence with the debug reads on."""
    case = R.BY_NAME[name]
    base = runs.run(case)
    got = runs.run(case, debug=False, knobs=knobs, keep=False)
    reached = {k: got['forms'][k] for k in want}
    assert reached == want, (name, form, got['forms'])
    assert _scans.same_bits(got['RVEL'], base['RVEL']), '%s %s: %s' % (name, form, _scans.where_differs(got['RVEL'], base['RVEL']))
    assert np.isfinite(base['RVEL']).sum() > 0


def test_single_beam_kernel_with_melting_species_gives_the_same_bits(runs):
    """(E): CPOL_GATE1=2 takes the single-beam kernel with melting species, which diagnoses the melting layer itself: the melting
    case without its given fields (the general sequence with the debug reads on, and the default, which keeps k_gate1 off)."""
    case = R.BY_NAME['melt_g257_s1_r8_p0']
    base = runs.run(case, diagnose=True)
    assert base['forms']['gate1'] == 0 and np.isfinite(base['RVEL']).sum() > 1000
    for knobs, gate1 in (((), 0), (_knobs(CPOL_GATE1=2), 1)):
        got = runs.run(case, debug=False, knobs=knobs, keep=False, diagnose=True)
        assert got['forms']['gate1'] == gate1, got['forms']
        assert _scans.same_bits(got['RVEL'], base['RVEL']), (knobs, _scans.where_differs(got['RVEL'], base['RVEL']))


def test_final_512_gives_the_same_bits(runs, tmp_path):
    """(E): k_final with 256 and with 512 threads.  Beyond 256 gates this process takes 512 threads for these ray counts
    (asserted from the rule's own numbers); CPOL_FINAL_512 is read once per process, so a child takes 256."""
    import subprocess
    import sys
    names = ['rsgi_g257_s3_r8_p0', 'melt_g257_s1_r8_p0', 'rsgi_g5460_s1_r1_p2']
    assert all(R.BY_NAME[k].n_gates > 256 and R.BY_NAME[k].n_rays <= 256 for k in names) and 'CPOL_FINAL_512' not in os.environ
    code = ('import sys, numpy as np\n'
            'sys.path[:0] = %r\n'
            'import _rvel as R\n'
            'import test_gpu_rvel as T\n'
            'r = T.Runs()\n'
            'np.savez(sys.argv[1], **{k: r.run(R.BY_NAME[k], debug=False)["RVEL"] for k in %r})\n'
            'r.close()\n') % ([p for p in sys.path if p], names)
    out = str(tmp_path / 'final256.npz')
    env = dict({k: x for k, x in os.environ.items() if k not in KNOBS}, CPOL_FINAL_512='0')
    p = subprocess.run([sys.executable, '-c', code, out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(out)
    for k in names:
        here = runs.run(R.BY_NAME[k], debug=False, keep=False)['RVEL']
        assert _scans.same_bits(got[k], here) and _scans.same_bits(here, runs.run(R.BY_NAME[k])['RVEL']), k


# --------------------------------------------------------------------------------------------------------------------- (F) folding
@pytest.fixture(scope='module')
def nyquist_file(tmp_path_factory):
    fn = tmp_path_factory.mktemp('nyquist') / 'nyquist.csv'
    fn.write_text(R.nyquist_text())
    return str(fn)


@pytest.mark.parametrize('case', R.ALIAS_CASES, ids=_ids(R.ALIAS_CASES))
def test_folding_is_the_formula_on_the_unfolded_run(runs, nyquist_file, case):
    """(F).  theta = (rv + nyq) / (2 nyq) pi - pi / 2 is rounded at |theta| 2^-53 (a few roundings), atan(tan(.)) does not amplify
    away from the poles (its derivative is 1) and the way back scales by 2 nyq / pi: a few units of 2^-53 (|rv| + nyq); 16."""
    unfolded = runs.run(case)['RVEL']
    folded = runs.run(case, nyquist_file=nyquist_file)['RVEL']
    nyq = R.nyquist_of(case)[:, None]
    assert len(np.unique(nyq)) >= 4
    want = R.alias(unfolded, nyq)
    assert np.array_equal(np.isnan(folded), np.isnan(unfolded)) and np.isnan(folded).any()
    ok = ~np.isnan(unfolded)
    bound = np.broadcast_to(16 * 2.0 ** -53 * (np.abs(unfolded) + nyq), unfolded.shape)
    err = np.abs(folded - want)
    assert (R.pole_distance(R.alias_theta(unfolded, nyq))[ok] > R.POLE_MARGIN).all()
    assert (err[ok] <= bound[ok]).all(), (case.name, float((err[ok] / bound[ok]).max()))
    assert (np.abs(folded[ok]) <= np.broadcast_to(nyq * (1 + 2.0 ** -50), folded.shape)[ok]).all()
    intervals = np.abs(unfolded[ok]) / np.broadcast_to(nyq, unfolded.shape)[ok]
    assert intervals.max() > 5 and (folded[ok] != unfolded[ok]).sum() > 0.5 * ok.sum()
    _record(stage='F_folding', case=case.name, gates=int(ok.sum()), worst_share_of_bound=float((err[ok] / bound[ok]).max()),
            most_nyquist_intervals=float(intervals.max()))
