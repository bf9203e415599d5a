"""The core of Doppler scheme 3 -- k_spec_gate, k_spec_atten, k_spec_final (cosmo_pol_amd/csrc/cpol_spectrum.inl) -- at every bin
count, gate count, sub-beam count and species set of tests/_spectrum.py, through RadarOperator.simulate_columns.

The stages are separated without a hook:
  (a) raw, k_spec_gate: one sub-beam with weight 1.0 and attenuation off.  DSPECTRUM is then the float32 beam widened (asserted:
      every value is a float32) and is compared with the oracle's subbeam_spectrum at PURE relative 2e-5, no atol, the support
      (> 0 and NaN patterns) bin for bin.  A bin beyond that is accepted only as one of a pair whose sum meets 2e-5 -- a table bin
      whose float32 edge diameter truncates to the neighbouring velocity bin (NumPy's float32 sin / tan against the device's
      correctly rounded ones) -- and only up to 5e-4 of a case's positive bins (never fewer than 4) and 1e-4 of the
      file's; tests/test_spectrum_cases_cpu.py shows that two host evaluations stay within half of both;
  (b) attenuation, k_spec_atten: the same columns with attenuation on.  From item_key / item_res of the run the front-aligned
      float64 sums of column 11 and their prefix sum are formed in NumPy, and from the raw rows of (a) every bin must equal
      float32(raw / frac) to within 4 float32 ulp (log10 and the power of 10 are the device's); a rank off by one moves a gate
      by far more.  The full result also against the oracle at 2e-5 under the pair rule;
  (c) accumulation, k_spec_final: every sub-beam alone gives its float32 beam exactly; float32(beam x float32(w)) -- per-gate
      weights: float32(float64(beam) x w) -- summed in float64 in sub-beam order must be the bits of the multi-sub-beam DSPECTRUM.
      RVEL against nansum(v acc) / nansum(acc) of the device's own spectrum within n_v 2^-53 sum|v acc| / sum acc (the order of
      the sums alone), NaN exactly where the oracle's is, and against the oracle at the suite's 2e-4 m/s;
  (d) the sensitivity cut: NaN exactly where NumPy's 10 log10(acc) < threshold(gate) holds (within 1e-4 dB either way), every
      other bin the uncut run's bits; gate 0 under a range-independent threshold;
  (e) limits: n_v above 4097 and an LDS request beyond 160 KB are CPOL_ERR_ARG, and the context repeats an earlier case bit for bit.
The worst deviations and the excepted-bin counts are printed and, when CPOL_PARITY_DIR names a directory, appended to
spectrum_parity_records.jsonl there (profiles/ keeps a copy).

The oracle's spectra are taken under _spectrum.rounded_powers(): the three float32 powers of a melting species' PSD as the float64
value rounded once.  NumPy's own float32 power is the loop the host CPU dispatches to; with AVX-512 it differs from the correctly
rounded value -- which C's powf gives but for one argument in a thousand, and which the device computes -- in the last bit of a
fifth of the arguments, and the finite difference in get_N turns such a bit into up to 7e-5 of a table entry.  Measured against the
oracle with the host's power (a host with AVX-512): 69 of 16 669 positive bins beyond 2e-5 at FFT 512 and 107 of 19 031 at FFT 2048
(2 and 6 of them not as a pair; the first of those off by 2.2e-5 and 3.5e-5), 170 of the file's 223 254, every one in a case with a melting species; two HOST
evaluations, one with each power, differ by the same 67 bins at FFT 512.  With the rounded powers the device gives the oracle's
bits in every positive bin of the file but 6 (three moved-edge pairs).
In (b) the gate's power s is summed in the wavefront's order (_spectrum.wave_nansum32): 10 log10 s is rounded to float32, whose
last bit is 15 ulp of every bin of the gate, and np.nansum -- another order -- moved whole gates by 6 to 14 ulp.  In the device's
order the deviation is 0 ulp on all 18 654 attenuated gates; the 4 ulp stay as the bound.

Tried against scratch builds of the library with one edit each, every index kept inside its buffer (89 tests; all pass on the
library as it is):
  * the chunk carry of the rank dropped (k_spec_atten: `rank = popcount(...)` without `count +`): 26 fail --
    test_attenuation_is_front_aligned in every case beyond 64 gates (20 of 26; 1, 2, 33, 63 and 64 gates pass), hundreds of bins
    beyond 4 ulp FROM GATE 0 ON (the 65th valid gate's attenuation lands on gate 0 and the prefix sum carries it along), and
    test_accumulation_carries_the_bits_of_the_definition's oracle comparison in the 6 cases beyond 64 gates.  The raw stage and
    RVEL (a quotient: the gate's factor cancels) pass.
  * the row loop one row short (k_spec_gate: `v + 2 < n_v`): 74 fail -- test_raw_stage_meets_the_oracle in all 24 cases that
    have a top gate (not the 1- and 2-gate cases), first at bin n_v - 2 of gate 2 or 10 (0.0 against the oracle's power), at
    n_v = 17 as at 2049; with it the attenuation, accumulation and RVEL tests of those cases, the two-velocity-arrays and
    large-LDS tests.
  * the re-clamp starting at q = p + 1 (a species' own limits skipped): 81 fail -- the raw stage in all 26 cases, hundreds of
    bins each, and everything built on it.
  * the per-gate weight form using the scalar weight (k_spec_final: `b * (float)sub_w[s]` always): 2 fail --
    test_accumulation_carries_the_bits_of_the_definition in the two per-gate-weight cases (1322 of 8385 and 2800 of 16 640 bins of
    ray 0 differ); the other 87 pass, as they must.
  * rho0 taken from the gate itself (no density correction): 78 fail -- the raw stage in all 25 cases with more than one gate
    (at gate 0 the edit changes nothing: the 1-gate case passes), and everything built on it.
The sensitivity-cut and limit tests compare runs of the same library with each other and with NumPy's rule: they pass on all five,
as they should."""
import copy
import json
import os

import numpy as np
import pytest

import _cases
import _scans
import _spectrum as S
from cosmo_pol_oracle import scatter

pytestmark = pytest.mark.gpu

KNOBS = ('CPOL_GATE1', 'CPOL_GATE1_RAY', 'CPOL_GATE1_SPECIES', 'CPOL_FUSE_GATE1', 'CPOL_FUSE_CLASSIFY', 'CPOL_RARE_DIRECT', 'CPOL_SUBSUM',
         'CPOL_FINAL_512', 'CPOL_USE_GRAPH', 'CPOL_EXP_SKIP', 'CPOL_ITAB', 'CPOL_ITAB_MELT')
CONSTANT_SENSITIVITY = -10.0                             # dBZ at every range: can censor gate 0 (the range-dependent threshold there is -inf)
MULTI = [c for c in S.CASES if c.n_sub > 1]
CUT_CASES = [c for c in S.CASES if c.name in ('rsgi_f64_g1_s1_r6_p1', '2mom_f64_g2_s2_r6_p3', 'melt_f64_g65_s1_r6_p3', 'rsgi_f255_g65_s1_r6_p6',
                                              'rsg_f64_g64_s5_r4_p0', 'melt_f255_g65_s2_r3_p7_wgate', 'rsg_f257_g65_s1_r6_p8')]

def _ids(cases):
    return [c.name for c in cases]


def _record(**kw):
    print(json.dumps(kw))
    out = os.environ.get('CPOL_PARITY_DIR')
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'spectrum_parity_records.jsonl'), 'a') as f:
        f.write(json.dumps(kw) + '\n')


class Runs(object):
    """One operator per species set; FFT length, attenuation switch and sensitivity are set through its configuration (the tables
    stay).  Every run is kept."""

    def __init__(self):
        self.ops, self.in_force, self.kept, self.book = {}, {}, {}, {}

    def luts(self, sset):
        conf, _, _ = S.oracle_setup(sset, 64)
        return {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in S.SPECIES[sset]}

    def make_operator(self, sset, over, luts=None):
        from cosmo_pol_amd import RadarOperator
        with pytest.MonkeyPatch.context() as mp:
            for k in KNOBS:
                mp.delenv(k, raising=False)
            return RadarOperator(config=copy.deepcopy(over), luts=self.luts(sset) if luts is None else luts, output_variables='only_radar')

    def operator(self, sset, fft, attenuation, sensitivity=None):
        over = S.config_overrides(sset, fft, attenuation, sensitivity)
        key = (fft, attenuation, repr(sensitivity))
        if sset not in self.ops:
            self.ops[sset] = self.make_operator(sset, over)
        elif self.in_force[sset] != key:
            conf = self.ops[sset].config
            for sec, d in over.items():
                conf[sec].update(copy.deepcopy(d))
            self.ops[sset].config = conf
        self.in_force[sset] = key
        # (the configuration's checks are type-strict and replace a refused value by its default: what was asked for is in force)
        got = self.ops[sset].config
        assert got['radar']['FFT_length'] == fft and got['radar']['radial_resolution'] == S.RADIAL_RES and \
            got['radar']['sensitivity'] == over['radar']['sensitivity'] and got['microphysics']['with_attenuation'] == attenuation and \
            got['doppler']['scheme'] == 3 and not got['doppler']['turbulence_correction'] and not got['doppler']['motion_correction'], got
        return self.ops[sset]

    def run(self, case, attenuation, sub=None, weights='one', cut=False, sensitivity=None, lane=0, items=False, keep=True):
        """-> dict(DSPECTRUM [n_rays, n_gates, n_v], RVEL, and with items: item_key [n_hydro, n_rays, n_gates], item_res
        [n_hydro, n_rays, n_gates, 12]).  sub: that sub-beam alone (S.alone); None: the case as it is."""
        key = (case.name, attenuation, sub, weights if sub is not None else None, cut, repr(sensitivity), lane, items)
        if key in self.kept:
            return self.kept[key]
        op = self.operator(case.sset, case.fft, attenuation, sensitivity)
        cols = dict(S.make_columns(case)) if sub is None else S.alone(case, sub, weights)
        n_sub = case.n_sub if sub is None else 1
        ctx = op._lane(lane)
        ctx.enable_debug(bool(items))
        res = op.simulate_columns(cols, apply_sensitivity=cut, lane=lane)
        varray = S.oracle_setup(case.sset, case.fft)[2]
        assert np.array_equal(np.asarray(op.constants.VARRAY, dtype=np.float64), varray), case.name
        assert res['n_sub'] == n_sub and res['DSPECTRUM'].shape == (case.n_rays, case.n_gates, len(varray)), (case.name, res['DSPECTRUM'].shape)
        assert res['DSPECTRUM'].dtype == np.float64 and res['RVEL'].dtype == np.float64
        forms = ctx.launch_forms()
        assert forms['gate1'] == 0 and forms['n_sub'] == n_sub and forms.get('subbeam_sum', 0) == 0, (case.name, forms)
        out = {'DSPECTRUM': res['DSPECTRUM'], 'RVEL': res['RVEL']}
        if items:
            assert n_sub == 1
            nh, n_sbg = len(case.species), case.n_rays * case.n_gates
            out['item_key'] = ctx.debug_read('item_key', (nh, n_sbg), np.int32).reshape(nh, case.n_rays, case.n_gates)
            out['item_res'] = ctx.debug_read('item_res', (nh, n_sbg, 12), np.float64).reshape(nh, case.n_rays, case.n_gates, 12)
            ctx.enable_debug(False)
        if keep:
            self.kept[key] = out
        return out

    def constants(self, case):
        """(c_att, res_km) of k_spec_atten for the case's configuration."""
        op = self.ops[case.sset]
        return 4.343e-3 * 2 * float(op.constants.WAVELENGTH), op.config['radar']['radial_resolution'] / 1000.

    def close(self):
        for op in self.ops.values():
            op.close()
        self.ops = {}


@pytest.fixture(scope='module')
def runs():
    r = Runs()
    yield r
    r.close()


def _subs(case):
    return range(case.n_sub)


# ---------------------------------------------------------------------------------------------------------- (a) the raw stage
def _raw_stage(runs, case):
    """The comparison of every sub-beam of the case alone, attenuation off, with the oracle (kept: the file's cap needs all of them)."""
    if case.name in runs.book:
        return runs.book[case.name]
    tot = dict(case=case.name, n_v=0, positive=0, excepted=0, failed=0, worst=0.0, first=None)
    for sub in _subs(case):
        got = runs.run(case, 0, sub=sub)['DSPECTRUM']
        tot['n_v'] = got.shape[2]
        assert S.is_float32(got), (case.name, sub)       # the float32 beam, widened
        for ray in range(case.n_rays):
            want = S.oracle_raw(case, ray, sub)
            assert not np.isnan(want).any()
            c = S.compare_bins(got[ray], want)
            tot['positive'] += c['positive']
            tot['excepted'] += c['excepted']
            tot['failed'] += c['failed']
            tot['worst'] = max(tot['worst'], c['worst'])
            if c['first'] is not None and tot['first'] is None:
                tot['first'] = (sub, ray) + c['first']
            if case.kind(ray) in ('empty', 'mask0') and case.n_gates > 1:
                assert not got[ray].any() and not want.any(), (case.name, ray)         # an empty ray; rho0 NaN: no row anywhere
    runs.book[case.name] = tot
    return tot


@pytest.mark.parametrize('case', S.CASES, ids=_ids(S.CASES))
def test_raw_stage_meets_the_oracle(runs, case):
    """(a).  What sees a row loop one row short, a species packed into the wrong LDS row, a clamp that skips a column, rho0 from
    the wrong gate: each moves whole bins by far more than 2e-5."""
    t = _raw_stage(runs, case)
    _record(stage='raw', **t)
    assert t['failed'] == 0, t
    assert t['excepted'] <= S.case_cap(t['positive']), t
    if case.n_gates > 2:
        assert t['positive'] >= 50, t


def test_raw_stage_excepted_bins_of_the_file(runs):
    tot = dict(positive=0, excepted=0, worst=0.0)
    for case in S.CASES:
        t = _raw_stage(runs, case)
        tot['positive'] += t['positive']
        tot['excepted'] += t['excepted']
        tot['worst'] = max(tot['worst'], t['worst'])
    _record(stage='raw', case='the file', **tot)
    assert tot['positive'] > 200000 and tot['excepted'] <= S.CAP_FILE * tot['positive'], tot


def test_same_bin_count_from_two_velocity_arrays(runs):
    """FFT 63 and 64 give n_v = 65 from different velocity arrays: the same operator, one call after the other, each its own
    result (the raw-stage test compares both with the oracle) -- and the first again, bit for bit."""
    a, b = [c for c in S.BIN_CASES if c.fft == 63][0], [c for c in S.BIN_CASES if c.fft == 64][0]
    assert a.sset == b.sset
    first = runs.run(a, 0, sub=0, keep=False)['DSPECTRUM']
    other = runs.run(b, 0, sub=0, keep=False)['DSPECTRUM']
    again = runs.run(a, 0, sub=0, keep=False)['DSPECTRUM']
    assert first.shape[2] == other.shape[2] == 65
    assert _scans.same_bits(first, again) and _scans.same_bits(first, _raw_bits(runs, a))
    assert S.compare_bins(first[0], S.oracle_raw(a, 0, 0))['failed'] == 0 and S.compare_bins(other[0], S.oracle_raw(b, 0, 0))['failed'] == 0


def _raw_bits(runs, case):
    return runs.run(case, 0, sub=0)['DSPECTRUM']


def test_large_lds_request_between_small_cases():
    """Six species at FFT 2048 ask for about 100 KB of LDS (hipFuncSetAttribute): on a fresh context after a small case and before
    the same small case again, and once more on a forked lane -- the same bits everywhere, the small case unchanged."""
    r = Runs()
    try:
        small, large = [c for c in S.BIN_CASES if c.fft == 64][0], S.LARGE_LDS
        assert small.sset == large.sset == 'melt'
        before = r.run(small, 0, sub=0, keep=False)['DSPECTRUM']
        big = r.run(large, 0, sub=0, keep=False)['DSPECTRUM']
        after = r.run(small, 0, sub=0, keep=False)['DSPECTRUM']
        forked = r.run(large, 0, sub=0, lane=1, keep=False)['DSPECTRUM']
        forked_small = r.run(small, 0, sub=0, lane=1, keep=False)['DSPECTRUM']
        assert _scans.same_bits(before, after) and _scans.same_bits(before, forked_small)
        assert _scans.same_bits(big, forked)
        assert (big > 0).sum() > 10000
        for ray in range(large.n_rays):
            c = S.compare_bins(big[ray], S.oracle_raw(large, ray, 0))
            assert c['failed'] == 0 and c['excepted'] <= S.case_cap(c['positive']), c
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------ (b) attenuation
@pytest.mark.parametrize('case', S.CASES, ids=_ids(S.CASES))
def test_attenuation_is_front_aligned(runs, case):
    """(b).  Every sub-beam of the case alone with attenuation on."""
    worst_ulp, n_moved, tot = 0, 0, dict(positive=0, excepted=0, failed=0, worst=0.0)
    for sub in _subs(case):
        raw = runs.run(case, 0, sub=sub)['DSPECTRUM'].astype(np.float32)
        on = runs.run(case, 1, sub=sub, items=True)
        got = on['DSPECTRUM']
        assert S.is_float32(got), (case.name, sub)
        c_att, res_km = runs.constants(case)
        pres = S.presence(case, weights=False)           # (the sub-beam alone runs with the scalar weight 1.0)
        for ray in range(case.n_rays):
            keys = on['item_key'][:, ray]
            want_valid = np.stack([pres[h][ray, sub] for h in case.species])
            assert np.array_equal(keys >= 0, want_valid), (case.name, sub, ray)        # an item exactly where the columns say
            ahc = S.front_aligned(keys, on['item_res'][:, ray, :, 11], c_att, res_km)
            want = S.attenuate(raw[ray], ahc)
            d = S.ulp_distance(got[ray].astype(np.float32), want)
            worst_ulp = max(worst_ulp, int(d.max()))
            assert d.max() <= 4, '%s sub-beam %d ray %d (%s): %d bins beyond 4 ulp, first at gate %d' % (
                case.name, sub, ray, case.kind(ray), int((d > 4).sum()), int(np.argwhere(d > 4)[0][0]))
            n_moved += int((want != raw[ray]).any(axis=1).sum())
            o = S.oracle_observables(case, ray, subs=[sub], weights='one', attenuation=1)
            c = S.compare_bins(got[ray], o.values['DSPECTRUM'])
            for k in ('positive', 'excepted', 'failed'):
                tot[k] += c[k]
            tot['worst'] = max(tot['worst'], c['worst'])
            assert c['failed'] == 0, (case.name, sub, ray, c)
    _record(stage='attenuation', case=case.name, worst_ulp=worst_ulp, gates_attenuated=n_moved, **tot)
    assert tot['excepted'] <= S.case_cap(tot['positive']), tot
    assert n_moved > 0 or case.n_gates <= 2 or tot['positive'] == 0, case.name


# ----------------------------------------------------------------------------------------------------------- (c) accumulation
@pytest.mark.parametrize('case', MULTI, ids=_ids(MULTI))
def test_accumulation_carries_the_bits_of_the_definition(runs, case):
    """(c).  Attenuation on: the beams are the attenuated ones."""
    cols = S.make_columns(case)
    weights = 'gate01' if case.wgate else 'one'
    beams = np.stack([runs.run(case, 1, sub=s, weights=weights, items=not case.wgate)['DSPECTRUM'] for s in _subs(case)])
    assert S.is_float32(beams)
    beams = beams.astype(np.float32)                     # [n_sub, n_rays, n_gates, n_v]
    multi = runs.run(case, 1)
    varray = S.oracle_setup(case.sset, case.fft)[2]
    worst_rv, worst_share, tot = 0.0, 0.0, dict(positive=0, excepted=0, failed=0, worst=0.0)
    for ray in range(case.n_rays):
        w = cols['quad_weights'][ray] if case.wgate else cols['quad_weights']
        want = S.accumulate(beams[:, ray], w)
        got = multi['DSPECTRUM'][ray]
        assert _scans.same_bits(got, want), '%s ray %d: %s' % (case.name, ray, _scans.where_differs(got, want))
        rv, bound = S.rvel(got, varray)
        o = S.oracle_observables(case, ray, attenuation=1)
        assert np.array_equal(np.isnan(multi['RVEL'][ray]), np.isnan(o.values['RVEL'])), (case.name, ray)
        assert np.array_equal(np.isnan(multi['RVEL'][ray]), np.isnan(rv)), (case.name, ray)
        ok = ~np.isnan(rv)
        if ok.any():
            err = np.abs(multi['RVEL'][ray][ok] - rv[ok])
            assert (err <= bound[ok]).all(), (case.name, ray, float((err / bound[ok]).max()))
            worst_share = max(worst_share, float((err / np.maximum(bound[ok], 1e-300)).max()))
            worst_rv = max(worst_rv, float(np.abs(multi['RVEL'][ray][ok] - o.values['RVEL'][ok]).max()))
        c = S.compare_bins(got, o.values['DSPECTRUM'])
        for k in ('positive', 'excepted', 'failed'):
            tot[k] += c[k]
        tot['worst'] = max(tot['worst'], c['worst'])
        assert c['failed'] == 0, (case.name, ray, c)
    _record(stage='accumulation', case=case.name, worst_abs_RVEL=worst_rv, worst_share_of_RVEL_bound=worst_share, **tot)
    assert worst_rv <= 2e-4, worst_rv
    assert tot['excepted'] <= S.case_cap(tot['positive']) and tot['positive'] > (100 if case.n_gates > 2 else 0), tot


@pytest.mark.parametrize('case', [c for c in S.CASES if c.n_sub == 1], ids=_ids([c for c in S.CASES if c.n_sub == 1]))
def test_rvel_of_one_sub_beam(runs, case):
    """RVEL of the one-sub-beam cases (attenuation on): the lane-strided sums at every bin count, NaN where no bin holds power."""
    out = runs.run(case, 1, sub=0, items=True)
    varray = S.oracle_setup(case.sset, case.fft)[2]
    worst = 0.0
    for ray in range(case.n_rays):
        rv, bound = S.rvel(out['DSPECTRUM'][ray], varray)
        o = S.oracle_observables(case, ray, subs=[0], weights='one', attenuation=1)
        assert np.array_equal(np.isnan(out['RVEL'][ray]), np.isnan(o.values['RVEL'])), (case.name, ray)
        assert np.array_equal(np.isnan(out['RVEL'][ray]), np.isnan(rv)), (case.name, ray)
        ok = ~np.isnan(rv)
        if ok.any():
            assert (np.abs(out['RVEL'][ray][ok] - rv[ok]) <= bound[ok]).all(), (case.name, ray)
            worst = max(worst, float(np.abs(out['RVEL'][ray][ok] - o.values['RVEL'][ok]).max()))
    _record(stage='rvel', case=case.name, worst_abs_RVEL=worst)
    assert worst <= 2e-4, worst


# -------------------------------------------------------------------------------------------------------- (d) the sensitivity cut
def _assert_cut(cut, unc, thr, tag):
    """-> the censored bins.  A censored bin is NaN, every other bin has the uncut run's bits; the set is NumPy's but for the bins
    within 1e-4 dB of the threshold."""
    censored = np.isnan(cut) & ~np.isnan(unc)
    assert _scans.same_bits(cut[~censored], unc[~censored]), (tag, _scans.where_differs(cut[~censored], unc[~censored]))
    with np.errstate(invalid='ignore', divide='ignore'):
        db = 10 * np.log10(unc)
        want = db < thr[None, :, None]
        near = np.abs(db - thr[None, :, None]) <= 1e-4
    assert near.sum() <= 0.01 * near.size, (tag, int(near.sum()))
    assert not ((censored != want) & ~near).any(), (tag, int(((censored != want) & ~near).sum()))
    return censored


@pytest.mark.parametrize('case', CUT_CASES, ids=_ids(CUT_CASES))
def test_sensitivity_cut_is_bin_wise(runs, case):
    """(d).  The range-dependent threshold is -inf at gate 0 (range 0): nothing is cut there, not even an empty bin; a constant
    threshold cuts gate 0 too.  Attenuation on, the case's own sub-beams and weights."""
    unc = runs.run(case, 1)['DSPECTRUM']
    conf = S.oracle_setup(case.sset, case.fft, 1)[0]
    thr = scatter.sensitivity_threshold(conf, case.n_gates)
    cut = runs.run(case, 1, cut=True, keep=False)['DSPECTRUM']
    censored = _assert_cut(cut, unc, thr, case.name)
    assert thr[0] == -np.inf and not censored[:, 0].any()
    if case.n_gates > 1:
        assert censored[:, 1:].any() and (~np.isnan(cut[:, 1:]) & (cut[:, 1:] > 0)).any(), case.name
        assert np.isnan(cut[:, 1:][unc[:, 1:] == 0]).all()           # (10 log10(0) = -inf is below every finite threshold)
    conf = S.oracle_setup(case.sset, case.fft, 1, CONSTANT_SENSITIVITY)[0]
    thr = scatter.sensitivity_threshold(conf, case.n_gates)
    assert (thr == CONSTANT_SENSITIVITY).all()
    unc2 = runs.run(case, 1, sensitivity=CONSTANT_SENSITIVITY, keep=False)['DSPECTRUM']
    assert _scans.same_bits(unc2, unc)
    cut = runs.run(case, 1, cut=True, sensitivity=CONSTANT_SENSITIVITY, keep=False)['DSPECTRUM']
    censored = _assert_cut(cut, unc, thr, case.name + ' constant threshold')
    assert censored[:, 0].any() and (cut[:, 0] > 0).any(), case.name
    _record(stage='cut', case=case.name, censored=int(censored.sum()), kept=int((cut > 0).sum()))


# --------------------------------------------------------------------------------------------------------------------- (e) limits
def test_limits_are_refused_and_the_context_goes_on(monkeypatch):
    """n_vbins = 4098 (the product's bound is 4097) and an LDS request beyond 160 KB (six species on tables of 1280 diameters at
    n_vbins = 4097: 168 KB) are CPOL_ERR_ARG -- a ValueError naming the limit -- and the same context then repeats an earlier case
    bit for bit.  No configuration reaches these counts (FFT_length ends at 2048): the call's parameters are edited on their way."""
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import synthetic
    case = [c for c in S.BIN_CASES if c.fft == 64][0]
    assert case.sset == 'melt'
    conf = S.oracle_setup(case.sset, case.fft)[0]
    monkeypatch.setattr(synthetic, 'NUM_DIAMETERS', 1280)
    luts = {h: synthetic.make_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme'], n_e=2) for h in case.species}
    monkeypatch.undo()
    assert luts['R'].value_table.shape[-2] == 1280
    r = Runs()
    real = N.Context.run_columns
    try:
        r.ops[case.sset] = r.make_operator(case.sset, S.config_overrides(case.sset, case.fft, 0), luts=luts)
        r.in_force[case.sset] = (case.fft, 0, repr(None))
        before = r.run(case, 0, sub=0, keep=False)
        assert (before['DSPECTRUM'] > 0).sum() > 500
        for n_v, words in ((4098, 'n_vbins in'), (4097, '160 KB')):
            long_varray = np.ascontiguousarray(np.linspace(-19.0, 19.0, n_v))

            def edited(self, params, columns, outputs, n_v=n_v, long_varray=long_varray):
                p, c = N.SweepParams.from_buffer_copy(params), N.Columns.from_buffer_copy(columns)
                p.n_vbins = n_v
                c.varray = long_varray.ctypes.data
                return real(self, p, c, outputs)
            monkeypatch.setattr(N.Context, 'run_columns', edited)
            with pytest.raises(ValueError, match=words):
                r.run(case, 0, sub=0, keep=False)
            monkeypatch.setattr(N.Context, 'run_columns', real)
            again = r.run(case, 0, sub=0, keep=False)
            for k in ('DSPECTRUM', 'RVEL'):
                assert _scans.same_bits(again[k], before[k]), (n_v, k)
    finally:
        monkeypatch.setattr(N.Context, 'run_columns', real)
        r.close()
