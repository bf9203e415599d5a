"""The range scans at every gate count, in every launch form and at the float32 edges (tests/_scans.py).

PHIDP = nan_cumsum(2 KDP) and the two nan_cumprods behind the attenuated ZDR are strictly sequential float32 scans.  On the device they
are scan_lds_wave_exact (63 shifted adds / multiplies per row of 64 gates, a carry from lane 63 into the next row) or
scan_lds_sequential (one lane), inside k_final<256>, k_final<512>, k_scan_rays and k_gate1_ray_scan, each with its own LDS layout and
loads.  Three comparisons, all bit for bit:
  * the two functions themselves (cpol_debug_scan) against the definition, on operand rows that hold signed zeros, subnormals, inf,
    NaN, products that run to zero, stick in the subnormals or overflow, and lone operands at the row boundaries;
  * every launch form against the definition applied to that same run's per-gate outputs (restate), the attenuation factors rebuilt
    with the device's own exp10 (cpol_debug_math op 8) -- rays with data-free gates at the row boundaries, an empty ray, a ray whose
    products cross the subnormal range and reach zero;
  * the single-beam launch forms against each other.
Then the oracle at the suite's tolerances on every ray at 64, 513, 1025 and N_MAX gates, the sensitivity cut against the uncensored
run and against NumPy, and the gate limit: N_MAX runs in every form, N_MAX + 1 is refused and the context goes on.

simulate_columns reaches every launch form (asserted through launch_forms() after every run), so no cube is needed; which of
k_final<256> / k_final<512> runs is the host's choice from the ray and gate counts (512 threads when n_rays <= 256 and n_gates > 256) and
is not reported: the 257-ray cases are what takes k_final<256> beyond 256 gates.

Tried against scratch builds with one edit each (what was expected, what happened; "every kernel test" = test_kernels_meet_the_definition
in all five forms, test_k_final_256_beyond_256_gates in all three, test_one_gate_beyond_the_limit_is_refused in all five):
  * the carry dropped (`row0 > 0` made false in scan_lds_wave_exact): expected to fail from 65 gates on.  It does: the hook's wave form,
    sum and product, first at 65 gates in gate 64 (the one-lane form passes, every count up to 64 passes); every kernel test, first
    at 65 gates in gate 64; the oracle test at 513, 1025 and N_MAX gates (64 gates pass).  The single-beam forms still equal each other
    -- they share the function -- and so do the forms of tests/test_gpu_gate_tiles.py at 497 gates: a comparison of forms cannot see it.
  * `.rept 62` for `.rept 63`: expected to fail from 64 gates on, in lane 63.  It does: the same tests, first at 64 gates in gate 63
    (63 gates pass); the oracle test also at 64 gates (one gate of ZDR, 4e-5).
  * `+0.0f` for `-0.0f` as the sum's identity: expected to be seen by the hook's signed-zero rows alone.  NO test sees it, those rows
    included, and none can: the identity sits in the lanes behind the last gate, values move from lane to lane towards HIGHER gates
    only, and the carry out of a partly filled row is never used -- the identity never reaches a stored value.  (It would matter to a
    variant that stores or carries those lanes; -0.0 stays the right constant.)
  * k_scan_rays' second branch reading `p_zh[0]` for `f.ZH[ii]`: expected to fail from 513 gates on.  It does, in the k_scan_rays form
    alone: test_kernels_meet_the_definition[scan_rays] first at 513 gates in gate 512 (ZDR), test_single_beam_forms_give_the_same_bits,
    the sensitivity cut (two gates censored differently) and the limit test of that form; 512 gates and every other form pass."""
import numpy as np
import pytest

import _cases
import _scans as S
from cosmo_pol_oracle import config as ocfg
from cosmo_pol_oracle import scatter

pytestmark = pytest.mark.gpu

RTOL = 1e-5
FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL']
CUT_FIELDS = ('ZH', 'ZV', 'KDP', 'RHOHV', 'ZDR', 'PHIDP', 'RVEL')       # what the sensitivity cut censors
KNOBS = ('CPOL_GATE1', 'CPOL_GATE1_RAY', 'CPOL_GATE1_SPECIES', 'CPOL_FUSE_GATE1', 'CPOL_FUSE_CLASSIFY', 'CPOL_RARE_DIRECT', 'CPOL_SUBSUM',
         'CPOL_FINAL_512', 'CPOL_USE_GRAPH', 'CPOL_EXP_SKIP')
# launch form -> (environment at context creation, what launch_forms() must say after every run)
FORMS = {
    'final': ({'CPOL_GATE1_RAY': '0'}, {'gate1': 1, 'gate1_ray': 0, 'g1r': 0, 'n_sub': 1}),       # single-beam gate kernel + k_final
    'scan_rays': ({'CPOL_GATE1_RAY': '1'}, {'gate1': 1, 'gate1_ray': 1, 'g1r': 1, 'n_sub': 1}),   # k_gate1_ray + k_scan_rays
    'ticket': ({'CPOL_GATE1_RAY': '3'}, {'gate1': 1, 'gate1_ray': 1, 'g1r': 3, 'n_sub': 1}),      # k_gate1_ray_scan
    'general': ({'CPOL_GATE1': '0'}, {'gate1': 0, 'gate1_ray': 0, 'n_sub': 1}),                   # the general sequence, one sub-beam
    'general4': ({}, {'gate1': 0, 'gate1_ray': 0, 'n_sub': 4, 'subbeam_sum': 1}),                 # ... four sub-beams
}
SINGLE = ('final', 'scan_rays', 'ticket', 'general')
CONSTANT_SENSITIVITY = 20.0                              # dBZ at every range: can censor gate 0 (the range-dependent threshold there is -inf)


def _cases_of(form):
    return S.CASES_4 if form == 'general4' else S.CASES_1


class Runs(object):
    """One operator per (launch form, sensitivity), created under the form's environment (read when the context is created);
    every run is kept, its launch form asserted."""

    def __init__(self):
        self.ops, self.kept = {}, {}
        self.luts = None

    def operator(self, form, sensitivity=None):
        key = (form, repr(sensitivity))
        if key not in self.ops:
            from cosmo_pol_amd import RadarOperator
            over = S.config_overrides(sensitivity)
            if self.luts is None:
                conf = ocfg.make_config(over)
                hl = ocfg.hydrometeor_list(conf)
                assert tuple(hl) == S.SPECIES
                self.luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in hl}
            with pytest.MonkeyPatch.context() as mp:
                for k in KNOBS:
                    mp.delenv(k, raising=False)
                for k, v in FORMS[form][0].items():
                    mp.setenv(k, v)
                self.ops[key] = RadarOperator(config=over, luts=self.luts, output_variables='only_radar')
            # (the configuration's checks are type-strict and replace a refused value by its default: what was asked for is in force)
            got = self.ops[key].config['radar']
            assert got['radial_resolution'] == S.RADIAL_RES and got['sensitivity'] == over['radar']['sensitivity'], got
        return self.ops[key]

    def run(self, form, case, cut=False, sensitivity=None, keep=True):
        key = (form, case.name, cut, repr(sensitivity))
        if key in self.kept:
            return self.kept[key]
        op = self.operator(form, sensitivity)
        res = op.simulate_columns(dict(S.make_columns(case)), apply_sensitivity=cut)
        forms = op._ctx.launch_forms()
        want = dict(FORMS[form][1], scan_form=1, graph_replayed=0)
        assert {k: forms[k] for k in want} == want, (form, case.name, forms)
        assert res['n_sub'] == case.n_sub and res['ZH'].shape == (case.n_rays, case.n_gates)
        out = {k: res[k] for k in FIELDS + ['mask']}
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
def ctx():
    from cosmo_pol_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------------ the functions
@pytest.mark.parametrize('mul', [False, True], ids=['sum', 'product'])
@pytest.mark.parametrize('form', [1, 0], ids=['wave', 'one_lane'])
def test_scan_functions_meet_the_definition(ctx, form, mul):
    """scan_lds_wave_exact (form 1) / scan_lds_sequential (form 0) through cpol_debug_scan == scan_definition bit for bit, NaN at the
    same places: every row family at every count.  What sees a flushed subnormal, a wrong identity or a lost carry directly."""
    n_rows = 0
    for n in S.GATE_COUNTS:
        x = S.hook_rows(n, mul)
        got = ctx.debug_scan(form, mul, x)
        want = S.scan_definition(x, mul)
        for i, f in enumerate(S.families(mul)):
            assert S.same_bits(got[i], want[i]), '%s of %s at %d gates, form %d: %s' % (
                'product' if mul else 'sum', f, n, form, S.where_differs(got[i], want[i]))
            n_rows += 1
    assert n_rows == 21 * len(S.families(mul))


def test_scan_hook_refuses_what_lds_cannot_hold(ctx):
    one = np.ones((1, 16384), dtype=np.float32)
    assert ctx.debug_scan(1, True, one).shape == one.shape           # 64 KB: the most
    for form, x in ((1, np.ones((1, 16385), dtype=np.float32)), (2, one[:, :8]), (-1, one[:, :8]), (1, np.ones((0, 8), dtype=np.float32)),
                    (1, np.ones((2, 0), dtype=np.float32))):
        with pytest.raises(ValueError):
            ctx.debug_scan(form, False, x)
    x = S.hook_rows(65, False)
    assert S.same_bits(ctx.debug_scan(1, False, x), S.scan_definition(x, False))      # the context goes on


# ------------------------------------------------------------------------------------------------- the kernels against the definition
def _device_factors(ctx, att, radial_res):
    """The per-gate factors with the device's own bits: exp10 as gate_finish calls it, on -0.1f * ATT * res_km formed in float32."""
    e = S.factor_exponents(att, radial_res)
    return ctx.debug_math(8, e.astype(np.float64).ravel()).astype(np.float32).reshape(att.shape)


def _assert_restated(ctx, out, tag):
    fh, fv = _device_factors(ctx, out['ATT_H'], S.RADIAL_RES), _device_factors(ctx, out['ATT_V'], S.RADIAL_RES)
    assert np.array_equal(np.isnan(fh), np.isnan(out['ATT_H'])) and np.array_equal(np.isnan(fv), np.isnan(out['ATT_V'])), tag
    phidp, zdr = S.restate(out, fh, fv, S.RADIAL_RES)
    assert S.same_bits(out['PHIDP'], phidp), '%s: PHIDP: %s' % (tag, S.where_differs(out['PHIDP'], phidp))
    assert S.same_bits(out['ZDR'], zdr), '%s: ZDR: %s' % (tag, S.where_differs(out['ZDR'], zdr))
    return fh, fv


def _assert_families(case, out, fh, fv, tag):
    """The run shows what its rays were built for: NaN exactly at the data-free gates, the strong ray's condition from the device's
    factors."""
    for r in range(case.n_rays):
        fam = case.family(r)
        free = S.data_free(fam, case.n_gates)
        for k in ('KDP', 'ATT_H', 'ATT_V', 'PHIDP', 'ZH'):
            assert np.array_equal(np.isnan(out[k][r]), free), (tag, r, fam, k)
        if fam == 'strong' and case.n_gates >= S.STRONG_FROM:
            assert S.strong_condition(fh[r], fv[r]) == [], (tag, r, S.strong_condition(fh[r], fv[r]))
            assert np.isnan(out['ZDR'][r]).any() and np.isfinite(out['ZDR'][r][:S.STRONG_LEAD]).all(), (tag, r)
        elif fam != 'strong':
            assert np.array_equal(np.isnan(out['ZDR'][r]), free), (tag, r, fam)


@pytest.mark.parametrize('form', list(FORMS))
def test_kernels_meet_the_definition(runs, ctx, form):
    """PHIDP and ZDR of a run == restate(that run's KDP, DELTA_HV, ZH, ZV, ATT_H, ATT_V) bit for bit, every count and ray family."""
    n_finite = 0
    for case in _cases_of(form):
        out = runs.run(form, case)
        tag = '%s %s' % (form, case.name)
        fh, fv = _assert_restated(ctx, out, tag)
        _assert_families(case, out, fh, fv, tag)
        n_finite += int(np.isfinite(out['PHIDP']).sum())
    assert n_finite > 50000, n_finite


@pytest.mark.parametrize('form', ['final', 'general', 'general4'])
def test_k_final_256_beyond_256_gates(runs, ctx, form):
    """257 rays at 257, 513 and 1025 gates: with more than 256 rays k_final<256> walks the gates (with fewer, k_final<512>)."""
    for case in (S.CASES_MANY_4 if form == 'general4' else S.CASES_MANY_1):
        assert case.n_rays > 256 and case.n_gates > 256
        out = runs.run(form, case, keep=(form != 'general4'))
        tag = '%s %s' % (form, case.name)
        fh, fv = _assert_restated(ctx, out, tag)
        _assert_families(case, out, fh, fv, tag)
    if form == 'general':
        for case in S.CASES_MANY_1:
            a, b = runs.run('final', case), runs.run('general', case)
            for k in FIELDS + ['mask']:
                assert S.same_bits(a[k], b[k]), (case.name, k, S.where_differs(a[k], b[k]))


# ------------------------------------------------------------------------------------------------------ the forms against each other
def test_single_beam_forms_give_the_same_bits(runs):
    for case in S.CASES_1:
        ref = runs.run(SINGLE[0], case)
        for form in SINGLE[1:]:
            got = runs.run(form, case)
            for k in FIELDS + ['mask']:
                assert S.same_bits(got[k], ref[k]), '%s against %s, %s: %s: %s' % (form, SINGLE[0], case.name, k, S.where_differs(got[k], ref[k]))


# --------------------------------------------------------------------------------------------------------------------------- the oracle
@pytest.fixture(scope='module')
def oracle_setup():
    conf = ocfg.make_config(S.config_overrides())
    ol = {h: _cases.as_oracle_lut(_cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']))
          for h in ocfg.hydrometeor_list(conf)}
    return conf, ol


@pytest.mark.parametrize('n_gates', S.ORACLE_COUNTS)
def test_one_sub_beam_against_the_oracle(runs, oracle_setup, n_gates):
    """Every ray (every family, the strong-attenuation ray included: the NaN pattern equal, ZDR within tolerance where finite) at
    the suite's tolerances: pure 1e-5, KDP / PHIDP / DELTA_HV with their operand-scaled atol (tests/test_gpu_seam.py::_tol)."""
    from test_gpu_seam import _tol
    conf, ol = oracle_setup
    case = [c for c in S.CASES_1 if c.n_gates == n_gates][0]
    out = runs.run('final', case)
    n_zdr_nan_strong = 0
    for ray in range(case.n_rays):
        tag = '%s ray %d (%s): ' % (case.name, ray, case.family(ray))
        o = scatter.radar_observables(S.oracle_subbeams(case, ray), ol, conf, return_sz=True)
        sz = np.nan_to_num(o.sz_total.astype(np.float64))
        for k in FIELDS:
            atol = 2e-4 if k == 'RVEL' else _tol(tag, k, sz, conf)
            _cases.assert_close_nan(out[k][ray], o.values[k], rtol=RTOL, atol=atol, name=tag + k)
        assert np.array_equal(out['mask'][ray], o.mask), tag
        if case.family(ray) == 'strong':
            n_zdr_nan_strong += int(np.isnan(o.values['ZDR']).sum())
    assert n_zdr_nan_strong > 0


# ------------------------------------------------------------------------------------------------------------------ the sensitivity cut
def _assert_cut(case, cut, unc, thr, tag):
    """-> the censored set.  A censored gate is NaN in CUT_FIELDS and nowhere else; every other gate has the uncensored run's bits."""
    censored = np.isnan(cut['ZH']) & ~np.isnan(unc['ZH'])
    for k in FIELDS + ['mask']:
        if k in CUT_FIELDS:
            assert np.isnan(cut[k][censored]).all(), (tag, k)
            assert S.same_bits(cut[k][~censored], unc[k][~censored]), (tag, k, S.where_differs(cut[k][~censored], unc[k][~censored]))
        else:
            assert S.same_bits(cut[k], unc[k]), (tag, k)
    # against NumPy: 10 * log10(ZH) (float32) < threshold(r) (float64); the sets may differ only within 1e-4 dB of the threshold
    with np.errstate(invalid='ignore', divide='ignore'):
        dbz = 10 * np.log10(unc['ZH'])
        assert dbz.dtype == np.float32
        want = dbz < thr[None, :]
        near = np.abs(dbz.astype(np.float64) - thr[None, :]) <= 1e-4
    share = near.sum() / float(near.size)
    assert share <= 0.01, (tag, share)
    assert not ((censored != want) & ~near).any(), (tag, int(((censored != want) & ~near).sum()))
    return censored


@pytest.mark.parametrize('form', list(FORMS))
def test_sensitivity_cut_leaves_the_other_gates_alone(runs, oracle_setup, form):
    """apply_sensitivity=True against the same case uncensored, every count.  The scans run over UNCENSORED operands: a gate behind a
    censored one keeps its bits.  The threshold rises with range and is -inf at gate 0 (range 0, quirk Q6), so at ONE gate nothing can be
    cut: asserted; from two gates on the set is neither empty nor everything.  The same set in every single-beam form."""
    conf, ol = oracle_setup
    n_censored = 0
    for case in _cases_of(form):
        unc = runs.run(form, case)
        cut = runs.run(form, case, cut=True, keep=False)
        thr = scatter.sensitivity_threshold(conf, case.n_gates)
        tag = '%s %s' % (form, case.name)
        censored = _assert_cut(case, cut, unc, thr, tag)
        runs.kept[('censored', form, case.name)] = censored
        if case.n_gates == 1:
            assert thr[0] == -np.inf and not censored.any(), tag
        else:
            assert censored.any() and not censored.all() and not censored[np.isfinite(unc['ZH'])].all(), tag
        if form in SINGLE and ('censored', SINGLE[0], case.name) in runs.kept:
            assert np.array_equal(censored, runs.kept[('censored', SINGLE[0], case.name)]), tag
        n_censored += int(censored.sum())
    assert n_censored > 1000, n_censored


def test_sensitivity_cut_with_one_threshold_for_every_range(runs):
    """A constant threshold can censor gate 0: one, two and 65 gates in every single-beam form -- neither no gate nor every gate, the
    same set in every form."""
    conf = ocfg.make_config(S.config_overrides(CONSTANT_SENSITIVITY))
    for case in [c for c in S.CASES_1 if c.n_gates in (1, 2, 65)]:
        sets = []
        for form in SINGLE:
            unc = runs.run(form, case)
            cut = runs.run(form, case, cut=True, sensitivity=CONSTANT_SENSITIVITY, keep=False)
            thr = scatter.sensitivity_threshold(conf, case.n_gates)
            assert (thr == CONSTANT_SENSITIVITY).all()
            sets.append(_assert_cut(case, cut, unc, thr, '%s %s constant threshold' % (form, case.name)))
            assert sets[-1].any() and not sets[-1][np.isfinite(unc['ZH'])].all(), (form, case.name)
            assert np.array_equal(sets[-1], sets[0]), (form, case.name)
        if case.n_gates == 1:
            assert sets[0][:, 0].any()


# ----------------------------------------------------------------------------------------------------------------------------- the limit
@pytest.mark.parametrize('form', list(FORMS))
def test_one_gate_beyond_the_limit_is_refused(runs, ctx, form):
    """N_MAX gates run in every form and meet the definition (test_kernels_meet_the_definition has them; asserted again here from the
    kept run); N_MAX + 1 is CPOL_ERR_ARG -- a ValueError naming the limit -- and the same context then repeats a small case bit for bit."""
    cases = _cases_of(form)
    assert cases[-1].n_gates == S.N_MAX
    top = runs.run(form, cases[-1])
    _assert_restated(ctx, top, '%s at the limit' % form)
    small = [c for c in cases if c.n_gates == 129][0]
    before = runs.run(form, small)
    over = S.SweepCase(S.N_MAX + 1, n_sub=small.n_sub, n_rays=2)
    op = runs.operator(form)
    with pytest.raises(ValueError, match='n_gates too large'):
        op.simulate_columns(dict(S.make_columns(over)), apply_sensitivity=False)
    again = op.simulate_columns(dict(S.make_columns(small)), apply_sensitivity=False)
    forms = op._ctx.launch_forms()
    assert {k: forms[k] for k in FORMS[form][1]} == FORMS[form][1], forms
    for k in FIELDS + ['mask']:
        assert S.same_bits(again[k], before[k]), (form, k)
