"""The range scans without a GPU (tests/_scans.py): the definition against NumPy and the oracle, the coverage of the hook's rows and
of the sweep cases, the restatement of PHIDP / ZDR against the golden radials of the reference, and the strong-attenuation ray's
condition from the oracle."""
import os
import re

import numpy as np
import pytest

import _cases
import _scans as S
from cosmo_pol_oracle import config as ocfg
from cosmo_pol_oracle import scatter


def test_the_gate_limit_is_one_constant():
    """N_MAX of the tests is CPOL_MAX_GATES of the header; the host compares n_gates with that name, _native.py mirrors it, and it is
    the most gates whose three scan rows fit 64 KB of LDS next to the 16 bytes kept for the scan kernels' static variables."""
    from cosmo_pol_amd import _native as N
    assert S.N_MAX == N.MAX_GATES
    text = open(os.path.join(S.ROOT, 'cosmo_pol_amd', 'csrc', 'cosmo_pol_hip.hip')).read()
    assert re.search(r'if \(ng > CPOL_MAX_GATES\)', text)
    static = int(re.search(r'^#define CPOL_SCAN_LDS_STATIC (\d+)$', text, flags=re.M).group(1))
    assert 3 * 4 * S.N_MAX + static <= 65536 < 3 * 4 * (S.N_MAX + 1) + static
    assert static >= 12                                  # k_gate1_ray_scan: s_lookup, s_last, s_done (cpol_create checks the compiler's figure)
    assert S.GATE_COUNTS[-1] == S.N_MAX and len(S.GATE_COUNTS) == 21


@pytest.mark.parametrize('mul', [False, True], ids=['sum', 'product'])
def test_definition_is_numpy_and_the_oracle(mul):
    """scan_definition == np.cumsum / np.cumprod on float32 bit for bit, on every row of the hook at every count; and == the oracle's
    nan_cumsum / nan_cumprod, which replace NaN by the identity first."""
    n_rows = 0
    for n in S.GATE_COUNTS:
        x = S.hook_rows(n, mul)
        want = S.scan_definition(x, mul)
        with np.errstate(over='ignore', under='ignore', invalid='ignore'):
            got = (np.cumprod if mul else np.cumsum)(x, axis=1)
            assert got.dtype == np.float32
            assert S.same_bits(got, want), (n, S.where_differs(got, want))
            for i, f in enumerate(S.families(mul)):
                o = (scatter.nan_cumprod if mul else scatter.nan_cumsum)(x[i].copy())
                clean = np.where(np.isnan(x[i]), np.float32(1 if mul else 0), x[i])
                assert o.dtype == np.float32 and S.same_bits(o, S.scan_definition(clean, mul)), (n, f)
                n_rows += 1
    assert n_rows == 21 * len(S.families(mul))


def test_hook_rows_cover_what_they_claim():
    assert S.hook_coverage_failures() == []
    for mul in (False, True):
        a, b = S.hook_row('decades', 129, mul), S.hook_row('decades', 129, mul)
        assert S.same_bits(a, b)                         # (from the name alone)


def test_sweep_cases_cover_what_they_claim():
    assert S.sweep_coverage_failures() == []


@pytest.mark.parametrize('name', list(_cases.RADIAL_CASES))
def test_restate_reproduces_the_golden_radials(golden, name):
    """PHIDP and ZDR of the reference's radials from their KDP, DELTA_HV, ZH, ZV, ATT_H and ATT_V.  PHIDP bit for bit on every
    radial.  ZDR on the attenuated ones (without attenuation ZDR is the ratio of the cross sections and no scan is involved):
    the factors are NumPy's float32 power here and were the reference's when the fixtures were written; measured on all 24 attenuated
    radials (2 090 gates), restate gives the fixtures' ZDR bit for bit -- no factor differs in its last bit -- so the tolerance is
    0: equal bits."""
    g = golden('radial_' + name)
    need = ['obs_' + k for k in ('KDP', 'DELTA_HV', 'ZH', 'ZV', 'ATT_H', 'ATT_V', 'PHIDP', 'ZDR')]
    assert all(k in g.files for k in need), [k for k in need if k not in g.files]      # (every radial fixture holds them)
    conf = ocfg.make_config(_cases.gen_golden.radial_case_inputs(name)[0])
    res = conf['radar']['radial_resolution']
    fields = {k: g['obs_' + k] for k in ('KDP', 'DELTA_HV', 'ZH', 'ZV')}
    fh, fv = S.numpy_factors(g['obs_ATT_H'], res), S.numpy_factors(g['obs_ATT_V'], res)
    phidp, zdr = S.restate(fields, fh, fv, res)
    assert S.same_bits(phidp, g['obs_PHIDP']), S.where_differs(phidp, g['obs_PHIDP'])
    assert np.isfinite(phidp).sum() > 10
    if conf['microphysics']['with_attenuation']:
        assert S.same_bits(zdr, g['obs_ZDR']), S.where_differs(zdr, g['obs_ZDR'])
        assert np.isfinite(zdr).sum() > 10
    # NumPy's own scans in place of the definition: the same
    phidp2, zdr2 = S.restate(fields, fh, fv, res, scan=lambda x, mul: (np.cumprod if mul else np.cumsum)(x, axis=-1))
    assert S.same_bits(phidp2, phidp) and S.same_bits(zdr2, zdr)


@pytest.fixture(scope='module')
def oracle_setup():
    conf = ocfg.make_config(S.config_overrides())
    hl = ocfg.hydrometeor_list(conf)
    assert tuple(hl) == S.SPECIES and conf['microphysics']['with_attenuation'] and conf['radar']['radial_resolution'] == S.RADIAL_RES
    ol = {h: _cases.as_oracle_lut(_cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme'])) for h in hl}
    return conf, ol


def test_strong_attenuation_ray_meets_its_condition(oracle_setup):
    """The oracle on the strong-attenuation ray's columns, one and four sub-beams, every count from 63 gates on: both running products
    have a normal gate, then subnormal gates, then exact zeros; ZDR is 0 / 0 = NaN from there on and the oracle's own PHIDP / ZDR are
    the restatement of its other fields."""
    conf, ol = oracle_setup
    n_cases = 0
    for case in S.CASES_1 + S.CASES_4:
        if case.n_gates < S.STRONG_FROM:
            continue
        ray = case.rays_of('strong')[0]
        o = scatter.radar_observables(S.oracle_subbeams(case, ray), ol, conf)
        v = o.values
        fh, fv = S.numpy_factors(v['ATT_H'], S.RADIAL_RES), S.numpy_factors(v['ATT_V'], S.RADIAL_RES)
        assert S.strong_condition(fh, fv) == [], (case.name, S.strong_condition(fh, fv))
        ph, pv = S.scan_definition(fh, True), S.scan_definition(fv, True)
        both_zero = (ph == 0) & (pv == 0)
        assert both_zero.any() and np.isnan(v['ZDR'][both_zero]).all() and np.isfinite(v['ZDR'][:S.STRONG_LEAD]).all(), case.name
        assert np.isfinite(v['ZH']).all() and np.isfinite(v['PHIDP']).all(), case.name
        phidp, zdr = S.restate({k: v[k] for k in ('KDP', 'DELTA_HV', 'ZH', 'ZV')}, fh, fv, S.RADIAL_RES)
        assert S.same_bits(phidp, v['PHIDP']) and S.same_bits(zdr, v['ZDR']), case.name
        n_cases += 1
    assert n_cases == 2 * sum(n >= S.STRONG_FROM for n in S.GATE_COUNTS)


def test_data_free_gates_give_the_identities(oracle_setup):
    """What the families are for: at a data-free gate of either kind the oracle's KDP and attenuations are NaN -- the scans take 0
    and 1 there -- and PHIDP / ZDR are NaN at that gate alone; an all-empty ray is NaN throughout."""
    conf, ol = oracle_setup
    case = S.SweepCase(129)
    for ray in range(case.n_rays):
        fam = case.family(ray)
        free = S.data_free(fam, case.n_gates)
        v = scatter.radar_observables(S.oracle_subbeams(case, ray), ol, conf).values
        for k in ('KDP', 'ATT_H', 'ATT_V', 'PHIDP', 'ZDR', 'ZH'):
            if fam == 'strong' and k == 'ZDR':
                continue
            assert np.array_equal(np.isnan(v[k]), free), (fam, k)
