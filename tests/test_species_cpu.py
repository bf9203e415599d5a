"""The rule of the hydrometeor contributions (cosmo_pol_amd/species.py: fields_of, dominant_of, constants_of, Species) on the
host: hand-made rows against a direct float32 transcription of the totals' statements (gate_finish, cpol_final.inl) written
out here, and the oracle's own per-species sums (radar_observables(..., return_sz=True)) against the oracle's totals."""
import numpy as np
import pytest

import _cases
from cosmo_pol_amd import species as SP
from cosmo_pol_oracle import beam, scatter
from cosmo_pol_oracle import constants as OK

F32 = np.float32
C = (F32(1.7e3), F32(3.1e-3), F32(0.107))          # c_zh, c_kdp, c_2w: any three float32 numbers
NAN = F32(np.nan)


def finish_row(t, c_zh, c_kdp, c_2w):
    """gate_finish (cpol_final.inl) for one row of twelve float32 sums, statement by statement, every operation float32."""
    t = [NAN if v == 0 else F32(v) for v in t]
    with np.errstate(all='ignore'):
        two_pi = F32(2 * 3.14159265358979323846)
        b = F32(F32(F32(t[0] - t[1]) - t[2]) + t[3])
        cc = F32(F32(F32(t[0] + t[1]) + t[2]) + t[3])
        xs_h, xs_v = F32(two_pi * b), F32(two_pi * cc)
        t47, t65 = F32(t[4] + t[7]), F32(t[6] - t[5])
        aa = F32(F32(t47 * t47) + F32(t65 * t65))
        return {'ZH': F32(c_zh * xs_h), 'ZV': F32(c_zh * xs_v), 'ZDR': F32(xs_h / xs_v), 'KDP': F32(c_kdp * F32(t[10] - t[8])),
                'ATT_H': F32(F32(4.343e-3) * F32(c_2w * t[11])), 'ATT_V': F32(F32(4.343e-3) * F32(c_2w * t[9])),
                'RHOHV': F32(np.sqrt(F32(aa / F32(b * cc)))),
                'DELTA_HV': F32(np.arctan2(np.float64(F32(t[5] - t[6])), np.float64(F32(-t[4] - t[7]))))}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def rows(n_gates, n_hydro, seed):
    rng = np.random.default_rng(seed)
    sz = rng.uniform(0.1, 2.0, (1, n_gates, n_hydro, 12)).astype(F32)
    sz[..., 0] += F32(6.0)                         # b > 0 and cc > 0: reflectivities of a physical species
    sz[..., 3] += F32(6.0)
    return sz


def test_literal_is_the_float32_nearest_to_the_decimal():
    # 4.343e-3f of the kernel is the decimal rounded once; float32(4.343e-3) rounds twice -- the same number here
    from fractions import Fraction
    x = Fraction('4.343e-3')
    f = F32(4.343e-3)
    near = [Fraction(float(v)) for v in (np.nextafter(f, F32(0)), f, np.nextafter(f, F32(1)))]
    assert min(near, key=lambda v: abs(v - x)) == near[1]


def test_one_species_alone_reproduces_the_totals_statements():
    sz = rows(40, 1, 1)
    sz[0, 3, 0, :] = [5, 1, 2, 9, -3, 0.5, 0.25, 4, 1.5, 0.75, 2.5, 0.125]
    sz[0, 4, 0, 5] = np.inf
    zh = np.ones((1, 40), dtype=F32)
    got = SP.fields_of(sz, zh, *C)
    for g in range(40):
        want = finish_row(sz[0, g, 0], *C)
        for k in ('ZH', 'ZV', 'KDP', 'ATT_H', 'ATT_V', 'RHOHV', 'DELTA_HV', 'ZDR'):
            assert bits(got[k][0, 0, g:g + 1])[0] == bits(np.array([want[k]], dtype=F32))[0], (g, k)
    assert np.all(got['present'] == 1) and np.all(got['dominant'] == 0)
    assert np.array_equal(got['share'], np.ones((1, 40), dtype=F32))
    for k in SP.FIELDS:
        assert got[k].shape == (1, 1, 40) and got[k].dtype == np.float32


def test_zeros_of_either_sign_read_as_absent():
    sz = rows(3, 2, 2)
    sz[0, 0, 1, :] = 0.0
    sz[0, 1, 1, :] = -0.0
    sz[0, 2, 0, 10] = -0.0                          # one column only: KDP of that species is lost, ZH is not
    got = SP.fields_of(sz, np.ones((1, 3), dtype=F32), *C)
    for g in (0, 1):
        for k in SP.FIELDS:
            assert np.isnan(got[k][1, 0, g]), (g, k)
        assert got['present'][0, g] == 1 and got['dominant'][0, g] == 0
    assert np.isnan(got['KDP'][0, 0, 2]) and np.isfinite(got['ZH'][0, 0, 2])
    assert got['present'][0, 2] == 3


def test_a_tie_for_dominant_keeps_the_lower_slot():
    sz = rows(2, 3, 3)
    sz[0, 0, 2] = sz[0, 0, 0]                       # slots 0 and 2 identical
    sz[0, 0, 1, :4] = [1, 0.5, 0.5, 1]              # ... and slot 1 smaller
    sz[0, 1, 1] = sz[0, 1, 2]
    sz[0, 1, 0, :4] = [1, 0.5, 0.5, 1]
    got = SP.fields_of(sz, np.ones((1, 2), dtype=F32), *C)
    assert got['ZH'][0, 0, 0] == got['ZH'][2, 0, 0] > got['ZH'][1, 0, 0]
    assert got['dominant'][0, 0] == 0
    assert got['ZH'][1, 0, 1] == got['ZH'][2, 0, 1] > got['ZH'][0, 0, 1]
    assert got['dominant'][0, 1] == 1
    assert np.all(got['present'] == 7)


def test_an_empty_gate_gives_255_nan_and_0():
    sz = rows(2, 3, 4)
    sz[0, 1] = np.nan
    got = SP.fields_of(sz, np.array([[1.0, np.nan]], dtype=F32), *C)
    assert got['dominant'][0, 1] == 255 and np.isnan(got['share'][0, 1]) and got['present'][0, 1] == 0
    assert got['dominant'][0, 0] != 255 and got['present'][0, 0] == 7


def test_a_censored_gate_keeps_three_fields_and_loses_the_rest():
    sz = rows(2, 2, 5)
    free = SP.fields_of(sz, np.ones((1, 2), dtype=F32), *C)
    cut = SP.fields_of(sz, np.array([[1.0, np.nan]], dtype=F32), *C)
    for k in ('ATT_H', 'ATT_V', 'DELTA_HV'):
        assert np.array_equal(bits(cut[k]), bits(free[k])), k
        assert np.all(np.isfinite(cut[k]))
    for k in SP.CUT_FIELDS:
        assert np.all(np.isnan(cut[k][:, 0, 1])), k
        assert np.array_equal(bits(cut[k][:, 0, 0]), bits(free[k][:, 0, 0])), k
    assert cut['present'][0, 1] == 0 and cut['dominant'][0, 1] == 255 and np.isnan(cut['share'][0, 1])
    assert cut['present'][0, 0] == 3


def test_a_negative_b_counts_as_the_rule_says():
    # ZH_j < 0 is present; it is taken when it comes first and gives way to any larger value; it enters the sum with its sign
    sz = rows(3, 2, 6)
    neg = [1, 4, 4, 1] + [0.5] * 8                 # b = -6
    sz[0, 0, 0, :] = neg                            # negative first, positive second: the second wins
    sz[0, 1, 1, :] = neg                            # positive first: stays
    sz[0, 2, 0, :] = neg                            # negative alone
    sz[0, 2, 1, :] = np.nan
    got = SP.fields_of(sz, np.ones((1, 3), dtype=F32), *C)
    assert got['ZH'][0, 0, 0] < 0 and got['ZH'][1, 0, 1] < 0
    assert list(got['present'][0]) == [3, 3, 1]
    assert list(got['dominant'][0]) == [1, 0, 0]
    for g, d in enumerate((1, 0, 0)):
        with np.errstate(all='ignore'):
            s = F32(0.0)
            for j in range(2):
                if got['present'][0, g] >> j & 1:
                    s = F32(s + got['ZH'][j, 0, g])
            assert bits(got['share'][0, g:g + 1])[0] == bits(np.array([got['ZH'][d, 0, g] / s], dtype=F32))[0]
    assert got['share'][0, 2] == 1.0
    assert got['share'][0, 0] > 1.0                 # the sum is smaller than its largest term


def test_dominant_of_is_the_tail_of_fields_of():
    sz = rows(17, 4, 7)
    sz[0, ::3, 1] = np.nan
    got = SP.fields_of(sz, np.ones((1, 17), dtype=F32), *C)
    tail = SP.dominant_of(got['ZH'])
    for k in ('present', 'dominant', 'share'):
        assert np.array_equal(bits(tail[k]), bits(got[k])), k


def test_species_refuses_unknown_fields_and_an_empty_request():
    with pytest.raises(ValueError, match='unknown field'):
        SP.Species(fields=('ZH', 'PHIDP'))
    with pytest.raises(ValueError, match='nothing asked for'):
        SP.Species(fields=(), dominant=False, raw=False)
    s = SP.Species(fields=('KDP', 'ZH'))
    assert s.fields == ('ZH', 'KDP') and s.dominant and not s.raw
    assert SP.Species(fields=(), dominant=False, raw=True).raw
    assert SP.Species('ZDR').fields == ('ZDR',)
    assert SP.names(['R', 'S', 'G']) == ('R', 'S', 'G')
    with pytest.raises(ValueError):
        SP.names([])
    with pytest.raises(ValueError):
        SP.names(list('abcdefghi'))


def test_constants_are_the_launch_sequences():
    wl, k2 = 0.05330, 0.93
    c_zh, c_kdp, c_2w = SP.constants_of(wl, k2)
    assert c_zh == F32(float(wl ** 4 / (np.pi ** 5 * k2))) and c_zh.dtype == np.float32
    assert c_kdp == F32(1e-3 * (180.0 / np.pi) * wl) and c_2w == F32(2 * wl)


# ---- the oracle's own rays ----
def oracle_ray(name):
    conf, az, el, ocube, luts, _ = _cases.radial_case(name)
    subs = beam.interpolate_radial(ocube, conf, az, el)
    o = scatter.radar_observables(subs, {h: _cases.as_oracle_lut(l) for h, l in luts.items()}, conf, return_sz=True)
    c = SP.constants_of(OK.Derived(conf).WAVELENGTH, conf['radar']['K_squared'])
    assert o.sz_integ.dtype == np.float32
    got = SP.fields_of(o.sz_integ[None], o.values['ZH'][None].astype(F32), *c)
    return o, got


def test_rain_alone_equals_the_oracles_totals():
    o, got = oracle_ray('c1_rain_rhi')
    # (the cube holds rain alone: the slots behind it are staged and stay empty)
    assert np.all(np.isnan(o.sz_integ[:, 1:])) and np.all(np.isnan(got['ZH'][1:]))
    assert set(got['dominant'][0]) <= {0, 255}
    # (ZDR: the total's is attenuated along the ray, the species' is the intrinsic ratio -- not the same quantity)
    for k in ('ZH', 'ZV', 'KDP', 'ATT_H', 'ATT_V', 'RHOHV', 'DELTA_HV'):
        _cases.assert_close_nan(got[k][0, 0], o.values[k], 1e-5, name=k)
    assert np.isfinite(got['ZH']).sum() > 50
    assert np.array_equal(got['present'][0] == 1, np.isfinite(o.values['ZH']))


def test_the_additive_fields_sum_to_the_oracles_totals():
    o, got = oracle_ray('c2_rsg')
    assert o.sz_integ.shape[1] == 3
    with np.errstate(all='ignore'):
        for k in ('ZH', 'KDP', 'ATT_H'):
            tot = np.nansum(got[k][:, 0].astype(np.float64), axis=0)
            tot[np.all(np.isnan(got[k][:, 0]), axis=0)] = np.nan
            _cases.assert_close_nan(tot, o.values[k], 1e-5, name=k)
    assert len(set(got['dominant'][0]) - {255}) >= 2, set(got['dominant'][0])
    assert np.isfinite(got['ZH']).sum() > 100
