"""The cases of the Doppler-spectrum pass (tests/_spectrum.py) without a GPU: what the cases must stage, shown on the oracle alone.

  * the coverage of the case list, from the columns;
  * every case fills at least 50 velocity bins (but the 1- and 2-gate cases) and has gates whose LAST row, v = n_v - 2, holds
    power (the spectrum of every eighth gate sits at the top of the velocity axis);
  * the reference's re-clamp quirk bites, NaN edges of a melting species occur, the rows with wh < 0 begin on both sides of v = 0
    (the folded elevation makes wh fall with v: within a gate they are the upper end of the velocity axis, and W of both signs moves
    where they begin to either side of the axis' middle);
  * the attenuation added to the r-th VALID gate differs from the attenuation added to the gate itself on both sides of a chunk
    boundary of k_spec_atten;
  * the edge bins.  The bin edges are truncations of float32 diameters, and NumPy's float32 sin / tan are not correctly rounded
    (DESIGN.md 4): a last-bit difference in the sine can move one table bin between two neighbouring velocity bins.  Every raw-stage
    case is evaluated twice on the host -- with NumPy's functions, and with the float64 value rounded once, which is what the device
    does -- and the bins that differ by more than 2e-5 are counted.  tests/test_gpu_spectrum.py accepts such bins (as pairs) up to
    5e-4 of a case's positive bins, never fewer than 4, and 1e-4 of the file's; here the two host evaluations must stay within
    HALF of both.  If a case does not, choose other seeds; the cap stays.
The oracle's spectra are taken under S.rounded_powers() throughout (see there and test_rounded_powers_change_the_melting_species_alone)."""
import numpy as np
import pytest

import _spectrum as S
from cosmo_pol_oracle import scatter
from cosmo_pol_oracle import spectrum as SP

BOOK = {}                                                # case name -> what evaluate() found


def evaluate(case):
    """Every sub-beam of every ray of the case with NumPy's sine (the oracle's own function) and with the rounded one (through
    the restatement, which counts what it meets; test_restated_diameters_are_the_oracles pins it to the oracle's)."""
    if case.name in BOOK:
        return BOOK[case.name]
    conf, ol, varray = S.oracle_setup(case.sset, case.fft)
    stats = {}
    out = dict(positive=0, differ=0, unpaired=0, stats=stats, per_gate=[], top_rows=0)
    for ray in range(case.n_rays):
        for sub in range(case.n_sub):
            own = S.oracle_raw(case, ray, sub)
            sb = S.oracle_subbeams(case, ray, subs=[sub], weights='one')[0]
            S.fold(sb.elev_profile)
            with S.oracle_variant(trig='rounded', stats=stats), S.rounded_powers():
                rounded = SP.subbeam_spectrum(sb, list(case.species), ol, conf, varray)
            c = S.compare_bins(rounded, own)
            out['positive'] += c['positive']
            out['differ'] += c['excepted'] + c['failed']
            out['unpaired'] += c['failed']
            out['top_rows'] += int((own[:, -2] > 0).sum())            # gates whose LAST row (v = n_v - 2, edge n_v - 1) holds power
            if case.kind(ray) not in ('empty', 'mask0') and case.elevation(ray) in (45.0, 75.0, 89.5):
                out['per_gate'].append(int((own > 0).sum(axis=1).max()))
    BOOK[case.name] = out
    return out


def test_cases_cover_what_they_claim():
    assert S.coverage_failures() == []
    a, b = S.make_columns(S.CASES[3]), S.make_columns(S.Case(S.CASES[3].sset, 64, 65, n_rays=6, rot=3))
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)          # (from the name alone)


def test_bin_counts_are_the_velocity_arrays():
    """n_v = len(VARRAY) is FFT_length + 1 or + 2 -- np.arange decides; 63 and 64 give the same count from different arrays."""
    n_v = {}
    for fft in S.FFT_LENGTHS:
        conf, ol, varray = S.oracle_setup(S.SET_OF_FFT[fft], fft)
        assert conf['radar']['FFT_length'] == fft and len(varray) in (fft + 1, fft + 2), (fft, len(varray))
        n_v[fft] = len(varray)
    counts = sorted(n_v.values())
    assert counts[0] <= 18 and counts[-1] >= 2049
    for edge in (S.WAVE, S.GATE_THREADS):                # both sides of a wavefront and of k_spec_gate's workgroup
        assert any(c < edge for c in counts) and any(c == edge or c == edge + 1 for c in counts) and any(c > edge + 1 for c in counts), edge
    assert any(c == S.GATE_THREADS for c in counts) and any(c == S.GATE_THREADS + 1 for c in counts) and any(c == S.GATE_THREADS + 2 for c in counts)
    a, b = S.oracle_setup(S.SET_OF_FFT[63], 63)[2], S.oracle_setup(S.SET_OF_FFT[64], 64)[2]
    assert len(a) == len(b) == 65 and not np.array_equal(a, b)
    assert len(S.oracle_setup(S.TOP.sset, S.TOP.fft)[2]) == 17


@pytest.mark.parametrize('case', S.CASES, ids=[c.name for c in S.CASES])
def test_edge_bins_stay_within_half_the_cap(case):
    """The two host evaluations differ in at most half of what the device test accepts; every case fills its bins."""
    e = evaluate(case)
    print('%s: %d positive bins, %d differ by more than %g between the two host evaluations (%d of them not as a pair); %s'
          % (case.name, e['positive'], e['differ'], S.RTOL, e['unpaired'], e['stats']))
    assert e['differ'] <= S.case_cap(e['positive']) // 2, (case.name, e['differ'], e['positive'])
    if case.n_gates > 2:
        assert e['positive'] >= 50, (case.name, e['positive'])
        assert e['top_rows'] >= 3, (case.name, e['top_rows'])          # the last row of k_spec_gate's loop holds power on some gates


def test_edge_bins_of_the_file_and_what_the_cases_stage():
    tot = dict(positive=0, differ=0)
    stats = {}
    for case in S.CASES:
        e = evaluate(case)
        for k in tot:
            tot[k] += e[k]
        for k, v in e['stats'].items():
            stats[k] = stats.get(k, 0) + v
        if case.melt:
            assert e['stats']['nan_edge_rows'] > 0 or case.n_gates <= 2, case.name      # NaN edges of a melting species, in every melting case
    print('the file: %d positive bins, %d differ; %s' % (tot['positive'], tot['differ'], stats))
    assert tot['differ'] <= 0.5 * S.CAP_FILE * tot['positive'], tot
    assert tot['positive'] > 200000
    # the rows with wh < 0 begin below and above v = 0 (down- and updraughts), each at a good share of the gates
    assert stats['neg_below_zero'] > 0.1 * stats['gates'] and stats['neg_above_zero'] > 0.1 * stats['gates'], stats
    assert stats['nan_edge_rows'] > 100, stats
    # the steep rays fill the bins: at FFT 256 and beyond the fullest gate of a ray holds at least a tenth of the axis
    for case in S.BIN_CASES:
        if case.fft >= 254:
            assert max(evaluate(case)['per_gate']) >= 0.1 * case.fft, (case.name, evaluate(case)['per_gate'])


def test_restated_diameters_are_the_oracles():
    """S.diameters with its defaults == the oracle's diameters_from_radial_velocity bit for bit (every case: evaluate() asserts it
    on whole spectra); here on the function's own results, a melting gate included."""
    case = S.BY_NAME['melt_f64_g65_s1_r6_p3']
    calls = []
    own = SP.diameters_from_radial_velocity

    def both(*a, **k):
        x, y = own(*a, **k), S.diameters(*a, **k)
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y))
        calls.append(len(x[2]))
        return x
    SP.diameters_from_radial_velocity = both
    try:
        conf, ol, varray = S.oracle_setup(case.sset, case.fft)
        sb = S.oracle_subbeams(case, 0, subs=[0], weights='one')[0]
        S.fold(sb.elev_profile)
        SP.subbeam_spectrum(sb, list(case.species), ol, conf, varray)
    finally:
        SP.diameters_from_radial_velocity = own
    assert len(calls) == case.n_gates and sum(calls) > 100


def test_rounded_powers_change_the_melting_species_alone():
    """S.rounded_powers(): the float32 powers of a melting species' PSD as the float64 value rounded once.  Without a melting
    species the oracle's spectrum keeps its bits; the rounded power is C's powf but for a few arguments in a thousand (glibc's is
    correctly rounded that often), whatever loop NumPy's float32 power takes on this host.  What the host's own power makes of a
    melting case is printed, not asserted: it differs from host to host -- with AVX-512 dozens of bins of the FFT-512 case move by
    more than 2e-5, which is why the reference is not evaluated that way."""
    import ctypes
    import ctypes.util
    case = S.BY_NAME['rsgi_f255_g65_s1_r6_p6']
    for ray in (2, 5):
        a, b = S.oracle_raw(case, ray, 0, 'host'), S.oracle_raw(case, ray, 0)
        assert np.array_equal(a, b) and (a > 0).sum() > 100, ray
    D = np.linspace(0.2, 15.0, 2000).astype(np.float32)
    assert np.array_equal(S.power32(D, 2), D * D) and np.array_equal(S.power32(D.astype(np.float64), 3.1), D.astype(np.float64) ** 3.1)
    name = ctypes.util.find_library('m')
    if name:
        powf = ctypes.CDLL(name).powf
        powf.restype, powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
        for b in (3.0, 3.1, 0.89):
            libm = np.array([powf(float(x), b) for x in D], dtype=np.float32)
            assert (S.power32(D, b) != libm).mean() <= 0.01, b
            print('D ** %g: NumPy differs from the rounded value at %d of %d arguments, powf at %d'
                  % (b, int((D ** b != S.power32(D, b)).sum()), len(D), int((libm != S.power32(D, b)).sum())))
    case = S.BY_NAME['melt_f512_g65_s1_r6_p10']
    c = S.compare_bins(S.oracle_raw(case, 0, 0, 'host'), S.oracle_raw(case, 0, 0))
    print('%s ray 0, the host\'s float32 power against the rounded one: %s' % (case.name, c))


def test_reclamp_quirk_bites():
    """The clamp of species i on the WHOLE matrix against the clamp on its own column: a different spectrum on many gates."""
    n_gates = 0
    for case in (S.BY_NAME['2mom_f254_g65_s1_r6_p5'], S.BY_NAME['melt_f256_g65_s1_r6_p7'], S.BY_NAME['rsgi_f255_g65_s1_r6_p6']):
        conf, ol, varray = S.oracle_setup(case.sset, case.fft)
        for ray in range(case.n_rays):
            if case.kind(ray) in ('empty', 'mask0'):
                continue
            sb = S.oracle_subbeams(case, ray, subs=[0], weights='one')[0]
            S.fold(sb.elev_profile)
            with S.oracle_variant(reclamp='own'), S.rounded_powers():
                alt = SP.subbeam_spectrum(sb, list(case.species), ol, conf, varray)
            n = int((alt != S.oracle_raw(case, ray, 0)).any(axis=1).sum())
            print('%s ray %d: %d gates differ without the re-clamp' % (case.name, ray, n))
            n_gates += n
    assert n_gates >= 20, n_gates


def test_oracle_observables_shortcut_is_the_oracle():
    """oracle_observables hands the cached sub-beam spectra to radar_observables: the same bits as the plain call."""
    case = S.BY_NAME['rsg_f64_g64_s5_r4_p0']
    conf, ol, _ = S.oracle_setup(case.sset, case.fft, 1)
    for ray in (0, 2):
        a = S.oracle_observables(case, ray)
        b = scatter.radar_observables(S.oracle_subbeams(case, ray), ol, conf)
        for k in ('DSPECTRUM', 'RVEL', 'ZH'):
            assert np.array_equal(a.values[k], b.values[k], equal_nan=True), (ray, k)
        assert (a.values['DSPECTRUM'] > 0).sum() > 100             # (not an empty comparison)


def test_front_aligned_attenuation_differs_from_gate_aligned():
    """The attenuation of a species' r-th valid gate is added to gate r (the reference's quirk).  On the rays whose species are
    absent here and there it differs from the attenuation added to the gate itself on at least 5 gates on each side of the chunk
    boundaries 64 and 128 of k_spec_atten -- a rank that loses its carry moves these gates."""
    from cosmo_pol_oracle import constants as K
    seen = set()
    for case in S.CASES:
        if case.n_gates < S.WAVE + 16 or case.n_gates > 1000 or case.wgate:
            continue
        conf, ol, _ = S.oracle_setup(case.sset, case.fft, 1)
        c_att, res_km = 4.343e-3 * 2 * K.Derived(conf).WAVELENGTH, S.RADIAL_RES / 1000.
        pres = S.presence(case)
        for ray in range(case.n_rays):
            if case.kind(ray) not in ('rotated', 'mask', 'zero_q'):
                continue
            o = S.oracle_observables(case, ray, subs=[0], weights='one', return_sz=True)
            col11 = np.nan_to_num(o.sz_integ[:, :, 11].T.astype(np.float64))          # [n_hydro, n_gates] (weight 1.0)
            keys = np.where(np.stack([pres[h][ray, 0] for h in case.species]), 0, -1)
            assert np.array_equal(keys >= 0, ~np.isnan(o.sz_integ[:, :, 11].T)), (case.name, ray)
            front = S.front_aligned(keys, col11, c_att, res_km)
            gate = np.cumsum((c_att * col11 * res_km).sum(axis=0))
            differs = np.abs(front - gate) > 1e-3 * np.abs(gate)
            for edge in (S.WAVE, 2 * S.WAVE):
                if case.n_gates >= edge + 16 and differs[edge - 16:edge].sum() >= 5 and differs[edge:edge + 16].sum() >= 5:
                    seen.add((edge, case.kind(ray)))
            # and the oracle's own spectrum is the front-aligned one
            raw = np.array(S.oracle_raw(case, ray, 0))
            want = S.attenuate(raw, front)
            got = o.values['DSPECTRUM']
            c = S.compare_bins(got, want)
            assert c['failed'] == 0 and c['excepted'] == 0, (case.name, ray, c)
    assert {e for e, _ in seen} == {S.WAVE, 2 * S.WAVE} and len(seen) >= 4, seen
