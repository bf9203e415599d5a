"""The bad-value radial fixtures (oracle/gen_golden.py: PLANTINGS, BAD_VALUE_CASES) hold what they are there for.

A fixture whose planting the ray never crosses, or whose gates are almost all NaN, lets every comparison pass on
emptiness.  The generator refuses to write such a fixture; these tests assert the same conditions again from the committed
files, and -- where the reference is present -- that regenerating a fixture reproduces the committed arrays."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _cases

GG = _cases.gen_golden
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_bad_value_case_is_a_radial_case_with_coverage_conditions():
    assert set(GG.BAD_VALUE_CASES) == set(GG.COVERAGE)
    assert set(GG.BAD_VALUE_CASES) <= set(_cases.RADIAL_CASES)
    for name, (base, plantings) in GG.PLANTINGS.items():
        assert _cases.RADIAL_CASES[name] is _cases.RADIAL_CASES[base]        # the base case's configuration, untouched
        assert plantings
    # every kind of planting the cases are there for is somewhere
    kinds = set()
    for base, plantings in GG.PLANTINGS.values():
        for var, value, r_lo, r_hi in plantings:
            assert 0 <= r_lo < r_hi
            kinds.add((var if var in ('U', 'W', 'T', 'RHO') else var[:2], 'neg' if value == 'neg' else
                       'nan' if np.isnan(value) else 'm9999' if value == -9999.0 else 'zero' if value == 0 else 'value'))
    for want in [('U', 'nan'), ('U', 'm9999'), ('W', 'nan'), ('T', 'nan'), ('RHO', 'nan'), ('T', 'value'), ('QR', 'nan'),
                 ('QS', 'neg'), ('QN', 'zero'), ('QN', 'neg'), ('QN', 'nan')]:
        assert want in kinds, want


@pytest.mark.parametrize('name', GG.BAD_VALUE_CASES)
def test_planting_changes_only_what_it_names(name):
    """The planted cube differs from the clean one in the planted variables alone, inside the rings alone."""
    planted = GG.radial_case_inputs(name)[3]
    clean = GG.radial_case_inputs(name, clean=True)[3]
    touched = {p[0] for p in GG.PLANTINGS.get(name, ('', []))[1]}
    for k, v in clean['data'].items():
        same = np.array_equal(planted['data'][k], v, equal_nan=True)
        assert same == (k not in touched), k
    assert np.array_equal(planted['zlevels'], clean['zlevels'])


@pytest.mark.parametrize('name', GG.BAD_VALUE_CASES)
def test_fixture_coverage(golden, name):
    g = golden('radial_' + name)
    bad, counts = GG.coverage_failures(name, g)
    print(name, {k: counts[k] for k in ['finite_ZH', 'n_gates'] + GG.COVERAGE[name]})
    assert not bad, bad
    assert 3 * counts['finite_ZH'] >= counts['n_gates']
    for k in GG.COVERAGE[name]:
        assert counts[k] >= GG.MIN_COUNT.get(k, GG.MIN_EFFECT_GATES), (k, counts[k])
    # a data-born mask sets EVERY variable of the gate to NaN (interpolation.py:410), in every stored sub-beam
    for tag in ('subc_', 'subf_'):
        masked = g[tag + 'mask'] != 0
        for k in g.files:
            if k.startswith(tag) and k[5:] in _cases.ORDER_2MOM:
                assert np.all(np.isnan(g[k][masked])), k
    if name in GG.PLANTINGS and int(g['n_sub']) == 1:
        # the same gates have mask 0 on the unplanted cube: the masks counted above are born from the data
        # (one sub-beam: the radial's mask is the sub-beam's; the mask of an integrated radial sums over the sub-beams)
        born = (g['obs_mask'] != 0) & (g['clean_obs_mask'] == 0)
        assert born.sum() == counts['mask_m1_data'] + counts['mask_p1_data']
        assert np.all(np.isnan(g['obs_ZH'][born]))
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'radial_%s.npz' % name))
    assert size <= 100 * 1024, size                      # (the largest radial fixture before these: 100 KB)


def test_clean_runs_of_the_fixtures_equal_their_base_fixtures(golden):
    """clean_obs_* of a planted fixture is the reference on the base case's cube: the base fixture's own output."""
    for name, (base, _) in GG.PLANTINGS.items():
        g, b = golden('radial_' + name), golden('radial_' + base)
        assert np.array_equal(g['clean_obs_mask'], b['obs_mask']), name
        for k in ('ZH', 'RVEL', 'DSPECTRUM'):
            if 'clean_obs_' + k in g.files:
                assert np.array_equal(g['clean_obs_' + k], b['obs_' + k], equal_nan=True), (name, k)


def _reference_present():
    import ref_shim                                       # oracle/ref_shim.py (imports nothing of the reference by itself)
    return ref_shim.reference_available() and os.path.exists(os.path.join(ROOT, 'oracle', '_ref', 'libinterp_ref.so'))


@pytest.mark.parametrize('name', GG.BAD_VALUE_CASES)
def test_regenerating_reproduces_the_fixture(golden, tmp_path, name):
    if not _reference_present():
        pytest.skip('the reference (or oracle/_ref) is not present: fixtures cannot be regenerated here')
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'oracle', 'gen_golden.py'), '--out', str(tmp_path),
                           '--only', 'radials', '--cases', name], stdout=subprocess.DEVNULL)
    new = np.load(os.path.join(str(tmp_path), 'radial_%s.npz' % name), allow_pickle=False)
    g = golden('radial_' + name)
    assert sorted(new.files) == sorted(g.files)
    for k in g.files:
        assert new[k].dtype == g[k].dtype and new[k].shape == g[k].shape, k
        assert new[k].tobytes() == g[k].tobytes(), k


# ---------------------------------------------------------------- the planted broadening cases (tests/_broadening.py)

def test_planted_broadening_fixtures_coverage(golden):
    """NaN in EDR under mask 0, and EDR lost to a mask born from NaN in U, with the turbulence switch on: the reference
    accepts both and leaves every sub-beam unbroadened (the switch is all or nothing per sub-beam), where the same
    configuration on the clean cube broadens all three."""
    import _broadening as B
    assert set(B.PLANTINGS) == set(B.CLEAN_TWIN) <= set(B.CASES)
    for name in B.PLANTINGS:
        assert B.CASES[name] == B.CASES[B.CLEAN_TWIN[name]]
        g, clean = golden('radial_' + name), golden('radial_' + B.CLEAN_TWIN[name])
        bad, c = B.coverage_failures(name, g, clean)
        print(name, c)
        assert not bad, bad
        assert c['switch'] == [0, 0, 0] and c['clean_switch'] == [1, 1, 1]
        for s in range(int(g['n_sub'])):
            assert np.array_equal(g['sub%d_spec_broad' % s], g['sub%d_spec_raw' % s])
            assert np.isfinite(g['sub%d_width' % s]).sum() >= 20          # ... although most widths are finite
        assert min(c['nan_edr_mask0'] if name == 'bad_d3_turb_edr' else c['mask_m1_data']) >= B.MIN_EFFECT_GATES
        assert c['rows_kept'] >= 20 and c['bins_kept'] >= 40 and 3 * c['finite_ZH'] >= c['n_gates']
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'radial_%s.npz' % name)) <= 100 * 1024
    # NaN EDR alone changes no mask and no polarimetric variable: only the spectrum loses its broadening
    g, clean = golden('radial_bad_d3_turb_edr'), golden('radial_d3_turb_motion_sub')
    assert np.array_equal(g['obs_mask'], clean['obs_mask'])
    assert np.array_equal(g['obs_ZH'], clean['obs_ZH'], equal_nan=True)


def test_regenerating_reproduces_the_planted_broadening_fixtures(golden, tmp_path):
    import _broadening as B
    if not _reference_present():
        pytest.skip('the reference (or oracle/_ref) is not present: fixtures cannot be regenerated here')
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'gen_golden_broadening.py'), '--out', str(tmp_path),
                           '--only'] + list(B.PLANTINGS), stdout=subprocess.DEVNULL)
    for name in B.PLANTINGS:
        new = np.load(os.path.join(str(tmp_path), 'radial_%s.npz' % name), allow_pickle=False)
        g = golden('radial_' + name)
        assert sorted(new.files) == sorted(g.files)
        for k in g.files:
            assert new[k].dtype == g[k].dtype and new[k].tobytes() == g[k].tobytes(), (name, k)
