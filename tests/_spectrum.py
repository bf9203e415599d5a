"""Inputs and plain restatements for the core of Doppler scheme 3 (k_spec_gate, k_spec_atten, k_spec_final,
cosmo_pol_amd/csrc/cpol_spectrum.inl).

What decides whether these kernels are right is the NUMBER OF VELOCITY BINS n_v (stride loops of 256 threads and of 64 lanes, the
row loop `v + 1 < n_v`, the dynamic LDS sized by n_hydro x (n_d + n_v) + n_v), the NUMBER OF GATES (the rank of a species' valid
gates: a ballot popcount plus a carry across chunks of 64 gates), WHICH SPECIES ARE PRESENT at a gate (only those are packed into
LDS: the packed index p is not the slot j) and the number and kind of sub-beam weights.  Here are
  * SETS: four species sets (1-moment R S G; with ice crystals; 2-moment R S G H I; 1-moment with the melting scheme and ice);
  * Case / CASES / make_columns(case): the dict RadarOperator.simulate_columns takes -- steep rays (the fall speeds decide the
    bins), W of both signs, every ray one kind of presence pattern, the per-species families rotated over the species;
  * oracle_subbeams / oracle_raw: the oracle's SubBeams of the same columns and subbeam_spectrum on one of them;
  * diameters(...): get_diameter_from_rad_vel restated with two switches -- the sine and tangent as NumPy's float32 functions or as
    the float64 value rounded once (what the device does), the clamp on the whole matrix (the reference's quirk) or on the species'
    own column -- and with counters for what a case stages; oracle_variant(...) puts it in the oracle's place;
  * compare_bins(got, want): the pure relative comparison with the pair rule for bins moved to a neighbour;
  * front_aligned / attenuate / accumulate: k_spec_atten and k_spec_final by their definitions, in NumPy;
  * coverage_failures(): what the case list must hold, from the columns alone.
tests/test_spectrum_cases_cpu.py states the conditions on the oracle alone; tests/test_gpu_spectrum.py pins the device."""
import contextlib
import copy
import functools
import zlib

import numpy as np

import _cases
import _scans

N_MAX = _scans.N_MAX                                     # CPOL_MAX_GATES
RADIAL_RES = 300                                         # (an int: the configuration's range check is type-strict)
WAVE = 64                                                # gates per chunk of k_spec_atten's rank, lanes of k_spec_final
GATE_THREADS = 256                                       # CPOL_SPEC_THREADS
RTOL = 2e-5                                              # the project's figure for the spectrum
CAP_CASE, CAP_CASE_MIN, CAP_FILE = 5e-4, 4, 1e-4         # excepted bins: share of a case's positive bins, its floor, share of the file's

# species set -> the radial case of oracle/gen_golden.py whose configuration it takes
SETS = {'rsg': 'd3_rsg', 'rsgi': 'd3_1mom_ice_sub', '2mom': 'd3_2mom_sub', 'melt': 'd3_melt_ice_sub'}
SPECIES = {'rsg': ('R', 'S', 'G'), 'rsgi': ('R', 'S', 'G', 'I'), '2mom': ('R', 'S', 'G', 'H', 'I'),
           'melt': ('R', 'S', 'G', 'mS', 'mG', 'I')}
MELTING = ('mS', 'mG')
# log-uniform ranges of the mass and number densities: those of the golden radials (tests/_buckets.py::Q_RANGE), the mass
# densities from 1e-6 up so that every present species fills bins
Q_RANGE = {'QR_v': (1.0e-6, 2.0e-3), 'QS_v': (1.0e-6, 9.1e-4), 'QG_v': (1.0e-6, 6.5e-4), 'QI_v': (1.0e-7, 1.9e-5),
           'QH_v': (3.3e-7, 6.4e-6), 'QmS_v': (4.1e-4, 2.2e-3), 'QmG_v': (1.0e-6, 6.5e-4),
           'QNR_v': (2.7e-2, 1.1e5), 'QNS_v': (2.8, 1.3e3), 'QNG_v': (2.3e-2, 9.2e2), 'QNH_v': (0.12, 3.2), 'QNI_v': (3.4e3, 5.0e5)}

FFT_LENGTHS = (16, 31, 63, 64, 127, 254, 255, 256, 257, 511, 512, 1024, 2048)
SET_OF_FFT = {16: 'rsg', 31: 'rsgi', 63: 'melt', 64: 'melt', 127: 'rsg', 254: '2mom', 255: 'rsgi', 256: 'melt', 257: 'rsg',
              511: 'rsgi', 512: 'melt', 1024: '2mom', 2048: 'melt'}
GATE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 193)
SUB_COUNTS = (1, 2, 3, 5, 9)
ELEVATIONS = (45.0, 89.5, 20.0, 75.0, 100.0, -5.0)       # degrees, as they come (100 and -5 are folded by the product: 80 and 5)
# every ray one kind.  'subsets': every non-empty subset of R, S, G on consecutive gates; 'rotated': every species its own family
# of SPECIES_FAMILIES; 'mask' / 'zero_q': data-free gates (mask +-1 with NaN values / zero mass densities) around the chunk
# boundaries, the other gates rotated; 'mask0': the same with gate 0 masked -- rho0 is NaN there and the whole ray's spectrum 0
RAY_KINDS = ('rotated', 'subsets', 'mask', 'all', 'zero_q', 'mask0', 'empty')
SPECIES_FAMILIES = ('front', 'row', 'every2', 'all', 'last')
FRONT_ABSENT = 6                                         # 'front': absent on gates 0 ... 5 (fewer on short rays)
TOP_WH = (1.0, 6.0)                                      # m/s: wh at the last velocity of a 'top' gate, before the density correction
FREE_GATES = (3, 61, 62, 64, 126, 127, 130)              # the data-free gates of 'mask' / 'zero_q' (and gate 0 of 'mask0')


@functools.lru_cache(maxsize=None)
def base_overrides(sset):
    over = _cases.gen_golden.radial_case_inputs(SETS[sset])[0]
    return {k: dict(v) for k, v in over.items()}


def config_overrides(sset, fft, attenuation, sensitivity=None):
    """The configuration of a run: the set's radial case with Doppler scheme 3, no broadening, this FFT length and attenuation
    switch; range-dependent sensitivity (10 dBZ at 10 km) unless given."""
    over = copy.deepcopy(base_overrides(sset))
    over['radar'].update(FFT_length=int(fft), radial_resolution=RADIAL_RES, sensitivity=[10, 10000] if sensitivity is None else sensitivity)
    over['microphysics']['with_attenuation'] = int(attenuation)
    over['doppler'] = {'scheme': 3, 'turbulence_correction': 0, 'motion_correction': 0}
    return over


def variable_names(sset):
    return tuple(_cases.ORDER_2MOM if sset == '2mom' else _cases.ORDER)


def q_name(h):
    return 'Q' + h + '_v'


class Case(object):
    """n_rays rays of n_sub sub-beams of n_gates gates under species set `sset` at FFT length `fft`.  Ray r is of kind
    RAY_KINDS[(r + rot) mod 7] at elevation ELEVATIONS[r mod 6]; `wgate`: per-gate weights with zeros (a 3-D quad_weights)."""

    def __init__(self, sset, fft, n_gates, n_sub=1, n_rays=6, rot=0, wgate=False):
        self.sset, self.fft, self.n_gates, self.n_sub, self.n_rays, self.rot, self.wgate = sset, fft, n_gates, n_sub, n_rays, rot, wgate
        self.species = SPECIES[sset]
        self.melt = sset == 'melt'
        self.name = '%s_f%d_g%d_s%d_r%d_p%d%s' % (sset, fft, n_gates, n_sub, n_rays, rot, '_wgate' if wgate else '')

    def kind(self, ray):
        return RAY_KINDS[(ray + self.rot) % len(RAY_KINDS)]

    def elevation(self, ray):
        return ELEVATIONS[ray % len(ELEVATIONS)]

    def family(self, ray, j):
        """The presence family of species slot j on a ray whose kind rotates them."""
        return SPECIES_FAMILIES[(ray + self.rot + 2 * j) % len(SPECIES_FAMILIES)]

    def __repr__(self):
        return self.name

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self.name == other.name


def _case_list():
    cases = []
    # every bin count at 65 gates (33 from FFT 1024 on), one sub-beam
    for i, fft in enumerate(FFT_LENGTHS):
        big = fft >= 1024
        # (three rays from FFT 1024 on: all / zero_q / mask0 at 1024, rotated / subsets / mask at 2048)
        cases.append(Case(SET_OF_FFT[fft], fft, 33 if big else 65, n_rays=3 if big else 6, rot={1024: 3, 2048: 0}.get(fft, i)))
    # every gate count at FFT 64, the sub-beam counts and the species sets in turn (65 gates: above, and nine sub-beams here)
    plan = ((1, 1, 'rsgi', 6, 1), (2, 2, '2mom', 6, 3), (63, 3, 'melt', 4, 5), (64, 5, 'rsg', 4, 0), (65, 9, 'rsgi', 3, 2), (127, 1, '2mom', 6, 4),
            (128, 2, 'melt', 4, 6), (129, 5, 'melt', 3, 1), (193, 1, 'rsg', 6, 0), (193, 3, 'rsgi', 3, 2))
    for ng, ns, sset, nr, rot in plan:
        cases.append(Case(sset, 64, ng, n_sub=ns, n_rays=nr, rot=rot))
    # per-gate weights with zeros
    cases.append(Case('rsgi', 64, 129, n_sub=3, n_rays=3, rot=0, wgate=True))
    cases.append(Case('melt', 255, 65, n_sub=2, n_rays=3, rot=7, wgate=True))
    # the most gates: k_spec_atten's dynamic LDS and serial prefix at their largest (n_v = 17, one ray of rotated families)
    cases.append(Case('rsg', 16, N_MAX, n_rays=1, rot=0))
    return tuple(cases)


CASES = _case_list()
BY_NAME = {c.name: c for c in CASES}
BIN_CASES = CASES[:len(FFT_LENGTHS)]
LARGE_LDS = [c for c in CASES if c.fft == 2048][0]          # six species at FFT 2048: about 100 KB of LDS, the hipFuncSetAttribute path
TOP = CASES[-1]


def sub_weights(n_sub):
    """Distinct and of one magnitude (tests/_subsum.py); one sub-beam: [1.0]."""
    s = np.arange(n_sub)
    return (1.0 + 0.4 * ((7 * s) % 131) / 131.0) / n_sub if n_sub > 1 else np.ones(1)


def velocity_array(sset, fft):
    from cosmo_pol_oracle import config as ocfg
    from cosmo_pol_oracle import spectrum as SP
    return SP.velocity_array(ocfg.make_config(config_overrides(sset, fft, 0)))


def top_gates(n_gates):
    """bool [n_gates]: the gates whose spectrum is put at the top of the velocity axis."""
    return np.arange(n_gates) % 8 == 2


def free_gates(kind, n_gates):
    """bool [n_gates]: the data-free gates of a ray of `kind`."""
    g = np.arange(n_gates)
    if kind == 'empty':
        return np.ones(n_gates, dtype=bool)
    if kind in ('mask', 'zero_q', 'mask0') and n_gates > 2:
        return np.isin(g, FREE_GATES + ((0,) if kind == 'mask0' else ()))
    if kind == 'mask0':
        return g == 0
    return np.zeros(n_gates, dtype=bool)


def family_pattern(family, n_gates):
    """bool [n_gates]: the gates at which a species of `family` is present."""
    g = np.arange(n_gates)
    if family == 'all':
        return np.ones(n_gates, dtype=bool)
    if family == 'front':
        return g >= min(FRONT_ABSENT, n_gates // 3)
    if family == 'row':                                  # absent on the whole second chunk
        return ~((g >= WAVE) & (g < 2 * WAVE))
    if family == 'every2':
        return g % 2 == 1 if n_gates > 1 else g == 0
    if family == 'last':
        return g == n_gates - 1
    raise ValueError(family)


def planned_presence(case, ray):
    """{species: bool [n_gates]} as the builder plans it (the same in every sub-beam)."""
    ng, kind = case.n_gates, case.kind(ray)
    g = np.arange(ng)
    out = {}
    for j, h in enumerate(case.species):
        if kind == 'all':
            p = np.ones(ng, dtype=bool)
        elif kind == 'empty':
            p = np.zeros(ng, dtype=bool)
        elif kind == 'subsets' and j < 3:
            p = (((g % 7) + 1) >> j) & 1 == 1            # R, S, G: the subsets 1 ... 7 on consecutive gates
        else:
            p = family_pattern(case.family(ray, j), ng)
        out[h] = p & ~free_gates(kind, ng)
    return out


@functools.lru_cache(maxsize=None)
def make_columns(case):
    """The columns of `case` (read-only arrays; computed once per case and shared)."""
    nr, ns, ng = case.n_rays, case.n_sub, case.n_gates
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    shape = (nr, ns, ng)
    names = variable_names(case.sset)
    cols = {}
    # winds of a few m/s -- the fall speeds decide the bins -- and W of both signs
    cols['U'] = (3.0 + 1.5 * rng.random(shape)).astype(np.float32)
    cols['V'] = (-2.0 - 1.5 * rng.random(shape)).astype(np.float32)
    cols['W'] = rng.uniform(-1.5, 1.5, shape).astype(np.float32)
    cols['RHO'] = (0.6 + 0.6 * rng.random((nr, 1, ng)) + 0.01 * rng.random(shape)).astype(np.float32)
    cols['T'] = (215.0 + 75.0 * rng.random((nr, 1, ng)) + rng.uniform(-1.0, 1.0, shape)).astype(np.float32)
    el_ray = np.array([case.elevation(r) for r in range(nr)])[:, None, None]
    el_sub = rng.uniform(-0.7, 0.7, (1, ns, 1)) if ns > 1 else np.zeros((1, 1, 1))
    az_sub = rng.uniform(-0.7, 0.7, (1, ns)) if ns > 1 else np.zeros((1, 1))
    cols['elev'] = (el_ray + el_sub + 0.01 * np.arange(ng)[None, None, :]).astype(np.float32)       # (89.5 deg crosses 90 at gate 50)
    cols['quad_pts'] = np.ascontiguousarray(np.stack(
        [np.broadcast_to(37.0 * np.arange(nr)[:, None] + az_sub, (nr, ns)), np.broadcast_to((el_ray + el_sub)[:, :, 0], (nr, ns))], axis=-1))
    # every eighth gate the spectrum sits at the TOP of the velocity axis: an updraught (steep rays) or a tail wind (the others) puts
    # wh(v_max) at TOP_WH m/s, so every row of the gate has wh >= 0 and the last row, v = n_v - 2, holds power
    top = top_gates(ng)
    if top.any():
        v_max = velocity_array(case.sset, case.fft)[-1]
        elf = fold(cols['elev'].astype(np.float64))
        th, phi = np.deg2rad(elf), np.deg2rad(cols['quad_pts'][:, :, 0])[:, :, None]
        U, V, W = (cols[k].astype(np.float64) for k in ('U', 'V', 'W'))
        t = rng.uniform(TOP_WH[0], TOP_WH[1], shape)
        w_top = v_max / np.sin(th) + t - (U * np.sin(phi) + V * np.cos(phi)) / np.tan(th)
        h_top = np.tan(th) * (v_max / np.sin(th) + t - W)
        steep = (elf >= 50.0) & top[None, None, :]
        flat = (elf < 50.0) & top[None, None, :]
        cols['W'] = np.where(steep, w_top, W).astype(np.float32)
        cols['U'] = np.where(flat, h_top * np.sin(phi), U).astype(np.float32)
        cols['V'] = np.where(flat, h_top * np.cos(phi), V).astype(np.float32)
    if case.wgate:
        w = sub_weights(ns)[None, :, None] * (1.0 + 0.2 * rng.random(shape))
        w[rng.random(shape) < 0.15] = 0.0
        cols['quad_weights'] = w
    else:
        cols['quad_weights'] = sub_weights(ns)
    for k in names:
        cols.setdefault(k, np.zeros(shape, dtype=np.float32))
    qs = [q_name(h) for h in case.species]
    for k in qs + (['QN' + h + '_v' for h in case.species] if case.sset == '2mom' else []):
        lo, hi = Q_RANGE[k]
        # log-uniform along the ray, within a factor of 2 across the sub-beams
        cols[k] = (np.exp(rng.uniform(np.log(lo), np.log(hi / 2), (nr, 1, ng))) * rng.uniform(1.0, 2.0, shape)).astype(np.float32)
    if case.melt:
        # the wet fractions run over the whole table axis along the ray: 1e-3 ... 0.999 (mS) and back (mG)
        t = np.arange(ng) / float(max(ng - 1, 1)) if ng > 1 else np.array([0.5])
        fw = 1e-3 * 999.0 ** t
        cols['fwet_mS'] = np.ascontiguousarray(np.broadcast_to(fw[None, None, :], shape) * rng.uniform(0.97, 1.0, shape)).clip(1e-3, 0.999)
        cols['fwet_mG'] = np.ascontiguousarray(np.broadcast_to(fw[::-1][None, None, :], shape) * rng.uniform(0.97, 1.0, shape)).clip(1e-3, 0.999)
        hm = np.ones((nr, ns), dtype=np.int8)
        hm[(np.arange(nr)[:, None] + np.arange(ns)[None, :]) % 4 == 1] = 0          # has_melting False on some sub-beams
        cols['has_melting'] = hm
    mask = np.zeros(shape, dtype=np.int8)
    for r in range(nr):
        kind = case.kind(r)
        free = free_gates(kind, ng)
        for h, p in planned_presence(case, r).items():
            cols[q_name(h)][r][:, ~p] = 0
        if kind in ('mask', 'mask0') and free.any():
            mask[r][:, free] = np.where(np.arange(int(free.sum())) % 2 == 0, 1, -1).astype(np.int8)      # (both codes, in turn)
            for k in names:
                cols[k][r][:, free] = np.nan
    cols['mask'] = mask
    for a in cols.values():
        a.setflags(write=False)
    return cols


def presence(case, cols=None, weights=True):
    """{species: bool [n_rays, n_sub, n_gates]} from the columns alone: Q > 0 (NaN is not), the sub-beam melts (mS / mG), the
    per-gate weight is > 0 (weights False: as in a call with scalar weights)."""
    cols = make_columns(case) if cols is None else cols
    out = {}
    for h in case.species:
        with np.errstate(invalid='ignore'):
            p = cols[q_name(h)] > 0
        if h in MELTING:
            p = p & (cols['has_melting'][:, :, None] != 0)
        if weights and np.ndim(cols['quad_weights']) == 3:
            p = p & (cols['quad_weights'] > 0)
        out[h] = p
    return out


def alone(case, sub, weights='one'):
    """The columns of sub-beam `sub` of the case as a call of its own.  weights 'one': the scalar weight 1.0; 'gate01': per-gate
    weights 1.0 where the case's are > 0 and 0.0 where they are 0 (a zero weight removes the gate's species, and with them ranks
    of k_spec_atten: the sub-beam alone must lose the same gates)."""
    cols = make_columns(case)
    out = {}
    for k, a in cols.items():
        if k == 'quad_weights':
            out[k] = np.ones(1) if weights == 'one' else (a[:, sub:sub + 1] > 0).astype(np.float64)
        elif k in ('quad_pts', 'has_melting') or np.ndim(a) == 3:
            out[k] = np.ascontiguousarray(a[:, sub:sub + 1])
        else:
            out[k] = a
    assert weights == 'one' or case.wgate
    return out


def fold(elev):
    """The in-place fold of doppler_scatter.py:173-176 as radar_observables applies it before the spectrum is formed."""
    elev[elev > 90] = 180 - elev[elev > 90]
    elev[elev < 0] = -elev[elev < 0]
    return elev


def oracle_subbeams(case, ray, subs=None, weights=None):
    """The oracle's sub-radials of one ray of the columns (fresh arrays: the oracle edits them in place).  weights 'one': every
    sub-beam with the scalar weight 1.0; 'gate01': see alone()."""
    from cosmo_pol_oracle.beam import SubBeam
    cols = make_columns(case)
    ng = case.n_gates
    w = cols['quad_weights']
    out = []
    for s in (range(case.n_sub) if subs is None else subs):
        values = {k: np.array(cols[k][ray, s], dtype=np.float32) for k in variable_names(case.sset)}
        if case.melt:
            for k in ('QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG'):
                values[k] = np.array(cols[k][ray, s], dtype=np.float64)
        if weights == 'one':
            qw = np.float64(1.0)
        elif weights == 'gate01':
            qw = (np.array(w[ray, s]) > 0).astype(np.float64)
        else:
            qw = np.array(w[ray, s]) if np.ndim(w) == 3 else np.float64(w[s])
        sb = SubBeam(values, cols['mask'][ray, s].astype(np.float64), np.zeros(ng), np.zeros(ng), float(RADIAL_RES) * (0.5 + np.arange(ng)),
                     np.zeros(ng), elev=np.array(cols['elev'][ray, s], dtype=np.float32), quad_pt=[float(x) for x in cols['quad_pts'][ray, s]],
                     quad_weight=qw)
        if case.melt:
            sb.has_melting = bool(cols['has_melting'][ray, s])
        out.append(sb)
    return out


@functools.lru_cache(maxsize=None)
def oracle_setup(sset, fft, attenuation=0, sensitivity=None):
    """-> (oracle configuration, {species: oracle table}, VARRAY)"""
    from cosmo_pol_oracle import config as ocfg
    from cosmo_pol_oracle import spectrum as SP
    sens = list(sensitivity) if isinstance(sensitivity, tuple) else sensitivity
    conf = ocfg.make_config(config_overrides(sset, fft, attenuation, sens))
    assert tuple(ocfg.hydrometeor_list(conf)) == SPECIES[sset]
    ol = {h: _cases.as_oracle_lut(_cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme'])) for h in SPECIES[sset]}
    return conf, ol, SP.velocity_array(conf)


def power32(D, b):
    """D ** b as the oracle writes it; for a float32 array the float64 value rounded once (x ** 2: the square)."""
    D = np.asarray(D)
    if D.dtype != np.float32:
        return D ** b
    if b == 2:
        return D * D
    return np.power(D.astype(np.float64), np.float64(np.float32(b))).astype(np.float32)


@contextlib.contextmanager
def rounded_powers():
    """The oracle with the float32 powers of a melting species' PSD -- a D^b, pi/6 D^3 and alpha D^beta on the float32 diameter grid
    (oracle/cosmo_pol_oracle/psd.py: get_M, get_V, _D_r; hydrometeors.py:372-439) -- taken as the float64 value rounded once.
    That is what the reference's platform gives (glibc's powf is correctly rounded but for about one argument in a thousand) and
    what the device does.  NumPy's own float32 power is whatever loop the host CPU dispatches to: with AVX-512 it differs from the
    correctly rounded value in the last bit of more than a fifth of the arguments, and the finite difference
    (D_r(D + 0.01) - D_r(D)) / 0.01 of get_N turns one such bit into up to 7e-5 of a table entry -- a reference evaluated that way
    carries an error of its own beyond the 2e-5 it is to judge, and another one on every host.  Nothing else changes: float64
    powers, every other statement and the other species (whose power tables the product takes from the host) stay as they are."""
    from cosmo_pol_oracle import psd
    own = psd.GammaPSD.get_M, psd.GammaPSD.get_V, psd.Melting._D_r

    def d_r(self, d):
        rho_m = self.get_M(d) / (np.pi / 6 * power32(d, 3))
        return (rho_m / psd.K.RHO_W) ** (1 / 3.) * d
    psd.GammaPSD.get_M = lambda self, D: self.a * power32(D, self.b)
    psd.GammaPSD.get_V = lambda self, D: self.alpha * power32(D, self.beta)
    psd.Melting._D_r = d_r
    try:
        yield
    finally:
        psd.GammaPSD.get_M, psd.GammaPSD.get_V, psd.Melting._D_r = own


@functools.lru_cache(maxsize=None)
def oracle_raw(case, ray, sub, powers='rounded'):
    """subbeam_spectrum of one sub-beam with the scalar weight 1.0, its elevations folded first -> float32 [n_gates, n_v]
    (read-only; computed once and shared).  powers 'rounded': under rounded_powers() (see there); 'host': NumPy's own."""
    from cosmo_pol_oracle import spectrum as SP
    conf, ol, varray = oracle_setup(case.sset, case.fft)
    sb = oracle_subbeams(case, ray, subs=[sub], weights='one')[0]
    fold(sb.elev_profile)
    with (rounded_powers() if powers == 'rounded' else contextlib.nullcontext()):
        raw = SP.subbeam_spectrum(sb, list(case.species), ol, conf, varray)
    raw.setflags(write=False)
    return raw


def oracle_observables(case, ray, subs=None, weights=None, attenuation=1, sensitivity=None, return_sz=False):
    """scatter.radar_observables on the sub-beams `subs` (all) of one ray.  With scalar weights the sub-beams' spectra come from
    oracle_raw (the same call on the same inputs, made once): the oracle goes on from there -- attenuation, weights, sum, RVEL."""
    from cosmo_pol_oracle import scatter
    from cosmo_pol_oracle import spectrum as SP
    sens = tuple(sensitivity) if isinstance(sensitivity, list) else sensitivity
    conf, ol, _ = oracle_setup(case.sset, case.fft, attenuation, sens)
    which = list(range(case.n_sub) if subs is None else subs)
    sbs = oracle_subbeams(case, ray, subs=which, weights=weights)
    if not np.isscalar(sbs[0].quad_weight):
        with rounded_powers():
            return scatter.radar_observables(sbs, ol, conf, return_sz=return_sz)
    queue = [np.array(oracle_raw(case, ray, s)) for s in which]
    own = SP.subbeam_spectrum
    SP.subbeam_spectrum = lambda *a, **k: queue.pop(0)
    try:
        return scatter.radar_observables(sbs, ol, conf, return_sz=return_sz)
    finally:
        SP.subbeam_spectrum = own


# --------------------------------------------------------------------------------------------- get_diameter_from_rad_vel, restated
def diameters(hyds, limits, varray, phi_deg, theta_deg, U, V, W, rho_corr, trig='numpy', reclamp='whole', stats=None):
    """oracle/cosmo_pol_oracle/spectrum.py::diameters_from_radial_velocity statement by statement, with
      trig    'numpy': np.tan / np.sin of the float32 angle (what the oracle and the reference do; NumPy's float32 functions
              are not correctly rounded); 'rounded': the float64 value rounded once to float32 (what the device does);
      reclamp 'whole': the clamp of species i on the WHOLE matrix (the reference's quirk); 'own': on its own column;
      stats   a dict of counters of what the call met."""
    theta = np.deg2rad(theta_deg)
    phi = np.deg2rad(phi_deg)
    if trig == 'rounded':
        tan_t, sin_t = np.float32(np.tan(np.float64(theta))), np.float32(np.sin(np.float64(theta)))
    else:
        tan_t, sin_t = np.tan(theta), np.sin(theta)
    with np.errstate(invalid='ignore', divide='ignore'):
        wh = (1. / rho_corr * (W + (U * np.sin(phi) + V * np.cos(phi)) / tan_t - varray / sin_t))
        idx = np.where(wh >= 0)[0]
        neg = wh < 0
        wh = wh[idx]
        D = np.zeros((len(idx), len(hyds)), dtype='float32')
        for i, h in enumerate(hyds):
            if hasattr(h, 'alpha'):
                D[:, i] = (wh / h.alpha) ** (1. / h.beta)
            else:
                from cosmo_pol_oracle import spectrum as SP
                D[:, i] = SP.melting_diameter_from_velocity(h, wh)
            d_min, d_max = limits[i]
            if reclamp == 'whole':
                D[D >= d_max] = d_max
                D[D <= d_min] = d_min
            else:
                col = D[:, i]
                col[col >= d_max] = d_max
                col[col <= d_min] = d_min
    Da = np.minimum(D[0:-1, :], D[1:, :])
    Db = np.maximum(D[0:-1, :], D[1:, :])
    mask = np.where(np.sum((Db - Da) == 0.0, axis=1) < len(hyds))[0]
    if stats is not None:
        v0 = varray[np.flatnonzero(neg)[0]] if neg.any() else np.inf           # the first velocity with wh < 0: the rows end there
        stats['gates'] = stats.get('gates', 0) + 1
        stats['neg_below_zero'] = stats.get('neg_below_zero', 0) + int(v0 < 0)
        stats['neg_above_zero'] = stats.get('neg_above_zero', 0) + int(0 < v0 < np.inf)
        stats['nan_edge_rows'] = stats.get('nan_edge_rows', 0) + int(np.isnan(Da[mask]).any(axis=1).sum())
        stats['rows'] = stats.get('rows', 0) + len(mask)
    return Da[mask, :], Db[mask, :], idx[mask]


@contextlib.contextmanager
def oracle_variant(**kw):
    """The oracle with diameters(..., **kw) in the place of its own diameters_from_radial_velocity."""
    from cosmo_pol_oracle import spectrum as SP
    own = SP.diameters_from_radial_velocity
    SP.diameters_from_radial_velocity = functools.partial(diameters, **kw)
    try:
        yield
    finally:
        SP.diameters_from_radial_velocity = own


# --------------------------------------------------------------------------------------------------------------- the comparison
def compare_bins(got, want, rtol=RTOL):
    """got, want: [n_gates, n_v].  Pure relative comparison bin for bin, no atol: a bin the reference leaves 0 must be 0, a NaN a
    NaN.  A bin beyond `rtol` is excepted only as one of a PAIR: the sum of it and an adjacent bin of the same gate meets `rtol`
    -- power moved to the neighbour (a table bin whose float32 edge diameter truncates to the other side), none was lost.
    -> dict(positive=bins > 0 in `want`, excepted=bins accepted by the pair rule, failed=the others beyond rtol, worst=the largest
    relative deviation among the bins within rtol, first=(gate, bin, got, want) of the first failure)."""
    a, b = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert a.shape == b.shape and a.ndim == 2, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.abs(a - b)
        bad = (err > rtol * np.abs(b)) | (na != nb)
        bad &= ~(na & nb)
        rel = np.where(b != 0, err / np.abs(b), 0.0)
    ok = ~bad & ~nb
    out = dict(positive=int((b > 0).sum()), excepted=0, failed=0, worst=float(rel[ok].max()) if ok.any() else 0.0, first=None)
    n_v = a.shape[1]
    for g, v in np.argwhere(bad):
        paired = False
        for u in (v - 1, v + 1):
            if 0 <= u < n_v and not (na[g, v] or nb[g, v] or na[g, u] or nb[g, u]):
                sa, sb = a[g, v] + a[g, u], b[g, v] + b[g, u]
                if abs(sa - sb) <= rtol * abs(sb):
                    paired = True
        if paired:
            out['excepted'] += 1
        else:
            out['failed'] += 1
            if out['first'] is None:
                out['first'] = (int(g), int(v), float(a[g, v]), float(b[g, v]))
    return out


def case_cap(positive):
    """The most excepted bins a case may have: 5e-4 of its positive bins, never fewer than 4."""
    return max(CAP_CASE_MIN, int(CAP_CASE * positive))


def is_float32(x):
    """Every value exactly representable in float32 (NaN counts)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        return bool(np.array_equal(x.astype(np.float32).astype(np.float64), x, equal_nan=True))


def ulp_distance(a, b):
    """|a - b| in units in the last place of float32, elementwise, for finite float32 a, b of one sign (0 where both are NaN)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    d = np.abs(ia - ib)
    d[np.isnan(a) & np.isnan(b)] = 0
    d[np.isnan(a) != np.isnan(b)] = 1 << 40
    return d


# ------------------------------------------------------------------------------------------------- k_spec_atten by its definition
def front_aligned(keys, col11, c_att, res_km):
    """keys [n_hydro, n_gates] (>= 0: the species has an item at the gate), col11 [n_hydro, n_gates] float64 (column 11 of its
    result) -> float64 [n_gates]: per species in slot order, the attenuation c_att * col11 * res_km of its r-th VALID gate (NaN
    counts as 0) added to gate r, then the prefix sum in gate order (doppler_scatter.py:297-305, 372-376)."""
    n_h, ng = keys.shape
    att = np.zeros(ng)
    for j in range(n_h):
        valid = keys[j] >= 0
        ah = c_att * col11[j][valid]
        ah = ah * res_km
        ah = np.where(np.isnan(ah), 0.0, ah)
        att[:len(ah)] = att[:len(ah)] + ah
    return np.cumsum(att)


def wave_nansum32(rows):
    """The float32 nansum of every row in the order of a wavefront: 64 lane sums over v = l, l + 64, ... in ascending order from
    +0.0, then the butterfly off = 32 ... 1 in which every lane adds its partner's value (IEEE addition commutes: every lane ends
    with the same bits)."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 2
    n, n_v = rows.shape
    pad = np.zeros((n, -(-n_v // WAVE) * WAVE), dtype=np.float32)
    pad[:, :n_v] = np.where(np.isnan(rows), np.float32(0), rows)
    pad = pad.reshape(n, -1, WAVE)
    s = np.zeros((n, WAVE), dtype=np.float32)
    for k in range(pad.shape[1]):
        s = s + pad[:, k]
    lane = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ off]
    assert s.dtype == np.float32 and (s == s[:, :1]).all()
    return s[:, 0]


def attenuate(raw, ahc, total=wave_nansum32):
    """raw float32 [n_gates, n_v] (a sub-beam's spectrum before the attenuation), ahc float64 [n_gates] -> float32: per gate
    s = float32 nansum of the row; where s > 0, frac = s / 10^(0.1 (float32(10 log10 s) - ahc)) and every bin float32(raw / frac).
    `total`: how s is summed -- in the device's order by default.  The order matters more than it seems: 10 log10 s is rounded
    to float32, whose last bit is up to 7.6e-6 dB = 1.8e-6 of frac = 15 float32 ulp of every bin of the gate, so an s that differs
    in its last bit moves a whole gate by that much whenever the rounding falls the other way."""
    raw = np.asarray(raw)
    assert raw.dtype == np.float32
    out = raw.copy()
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        s = total(raw)
        db = np.float32(10) * np.log10(s.astype(np.float64)).astype(np.float32)
        frac = s.astype(np.float64) / 10.0 ** (0.1 * (db.astype(np.float64) - ahc))
        on = s > 0
        out[on] = (raw[on].astype(np.float64) / frac[on, None]).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------- k_spec_final by its definition
def accumulate(beams, weights):
    """beams float32 [n_sub, n_gates, n_v]; weights [n_sub] (float32(beam x float32(w)): a float32 array times a Python float) or
    per gate [n_sub, n_gates] (float32(float64(beam) x w)); summed in float64 in sub-beam order from 0.0."""
    beams = np.asarray(beams)
    w = np.asarray(weights, dtype=np.float64)
    assert beams.dtype == np.float32 and w.shape[0] == beams.shape[0]
    acc = np.zeros(beams.shape[1:], dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for s in range(beams.shape[0]):
            if w.ndim == 1:
                wb = beams[s] * np.float32(w[s])
                assert wb.dtype == np.float32
            else:
                wb = (beams[s].astype(np.float64) * w[s][:, None]).astype(np.float32)
            acc = acc + wb.astype(np.float64)
    return acc


def rvel(acc, varray):
    """-> (nansum(v acc) / nansum(acc), the bound n_v 2^-53 sum|v acc| / sum acc on what another order of the sums can move it)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        num, den = np.nansum(varray[None, :] * acc, axis=1), np.nansum(acc, axis=1)
        bound = acc.shape[1] * 2.0 ** -53 * np.nansum(np.abs(varray[None, :] * acc), axis=1) / den
        return num / den, bound


# ------------------------------------------------------------------------------------------------------------------- the coverage
def coverage_failures():
    """What the case list must hold for the comparisons on the device to mean something, from the columns alone."""
    bad = []
    ffts = {c.fft for c in CASES if c.n_gates in (65, 33)}
    if ffts != set(FFT_LENGTHS) or any(c.n_gates > 33 for c in CASES if c.fft >= 1024):
        bad.append('bin counts: %s' % sorted(set(FFT_LENGTHS) - ffts))
    if {c.n_gates for c in CASES if c.fft == 64} != set(GATE_COUNTS):
        bad.append('gate counts at FFT 64')
    if not (TOP.n_gates == N_MAX and TOP.fft == 16 and TOP.n_rays == 1):
        bad.append('no case at the most gates')
    if {c.n_sub for c in CASES} != set(SUB_COUNTS):
        bad.append('sub-beam counts')
    if {c.sset for c in CASES} != set(SETS) or not (LARGE_LDS.fft == 2048 and len(LARGE_LDS.species) == 6):
        bad.append('species sets')
    seen = set()
    for c in CASES:
        cols = make_columns(c)
        pres = presence(c, cols)
        ng = c.n_gates
        w = cols['quad_weights']
        if c.n_sub > 1 and not c.wgate and (len(np.unique(w)) != c.n_sub or w.max() > 2 * w.min()):
            bad.append('%s: weights' % c.name)
        if c.wgate:
            if np.ndim(w) != 3 or not (w == 0).any() or (w == 0).all(axis=1).all():
                bad.append('%s: per-gate weights' % c.name)
            seen.add('wgate_zero')
        if c.melt:
            fw = cols['fwet_mS']
            if ng >= 63 and not (np.nanmin(fw) <= 1.1e-3 and np.nanmax(fw) >= 0.9):
                bad.append('%s: wet fraction %g ... %g' % (c.name, np.nanmin(fw), np.nanmax(fw)))
            if (cols['has_melting'] == 0).any() and (cols['has_melting'] != 0).any():
                seen.add('has_melting_false')
                if c.n_sub > 1 and ((cols['has_melting'] == 0).sum(axis=1) == 1).any():
                    seen.add('has_melting_false_on_one_sub_beam')
        for r in range(c.n_rays):
            kind = c.kind(r)
            el = c.elevation(r)
            seen.add(('elevation', el))
            free = free_gates(kind, ng)
            any_species = np.zeros((c.n_sub, ng), dtype=bool)
            for h in c.species:
                any_species |= pres[h][r]
            with np.errstate(invalid='ignore'):
                wpos = (w[r] > 0) if c.wgate else np.ones((c.n_sub, ng), dtype=bool)
            top = top_gates(ng) & ~(cols['mask'][r] != 0).any(axis=0)
            if top.any():
                th = np.deg2rad(fold(cols['elev'][r].astype(np.float64)))
                phi = np.deg2rad(cols['quad_pts'][r, :, 0])[:, None]
                U, V, W = (cols[k][r].astype(np.float64) for k in ('U', 'V', 'W'))
                wh = W + (U * np.sin(phi) + V * np.cos(phi)) / np.tan(th) - velocity_array(c.sset, c.fft)[-1] / np.sin(th)
                if not ((wh[:, top] > TOP_WH[0] - 0.1) & (wh[:, top] < TOP_WH[1] + 0.1)).all():
                    bad.append('%s ray %d: wh at the last velocity of the top gates: %s' % (c.name, r, wh[:, top]))
                seen.add('top')
            if (any_species & free[None, :]).any():
                bad.append('%s ray %d (%s): a species at a data-free gate' % (c.name, r, kind))
            by_mask = cols['mask'][r] != 0
            if kind in ('mask', 'mask0'):
                if not (by_mask == free[None, :]).all() or not np.isnan(cols['RHO'][r][:, free]).all():
                    bad.append('%s ray %d (%s): mask codes' % (c.name, r, kind))
                if free.sum() >= 2 and set(np.unique(cols['mask'][r])) != {-1, 0, 1}:
                    bad.append('%s ray %d (%s): both mask codes' % (c.name, r, kind))
                if kind == 'mask0' and free[0] and np.isnan(cols['RHO'][r][:, 0]).all() and ng > 1:
                    seen.add('rho0_nan')
                if kind == 'mask' and ng > 130:
                    seen.add('mask_gates')
            elif by_mask.any() or np.isnan(cols['RHO'][r]).any():
                bad.append('%s ray %d (%s): mask codes / NaN outside the mask kinds' % (c.name, r, kind))
            if kind == 'zero_q' and ng > 130 and free.sum() == len(FREE_GATES):
                seen.add('zero_q_gates')
            if kind == 'empty' and not any_species.any():
                seen.add('empty')
            if kind == 'all' and (any_species | ~wpos).all() and all((pres[h][r] | ~wpos).all() for h in c.species if h not in MELTING):
                seen.add('all')
            if kind == 'subsets' and ng >= 7:
                sub = sum((pres[h][r, 0].astype(int) << j) for j, h in enumerate(c.species[:3]))
                if not c.wgate and set(sub[:7].tolist()) == set(range(1, 8)):
                    seen.add('subsets')
                    # the packed index differs from the slot in every position: {S}, {G}, {R, G}, {S, G}
                    if {2, 4, 5, 6} <= set(sub.tolist()):
                        seen.add('packed_index_differs')
            if kind in ('rotated', 'mask', 'zero_q') and not c.wgate:
                for j, h in enumerate(c.species):
                    if h in MELTING and not cols['has_melting'][r, 0]:
                        continue
                    fam = c.family(r, j)
                    p = pres[h][r, 0]
                    if not np.array_equal(p, family_pattern(fam, ng) & ~free):
                        bad.append('%s ray %d: %s is not of family %s' % (c.name, r, h, fam))
                    if fam == 'front' and ng >= 63 and not p[:FRONT_ABSENT].any() and p[FRONT_ABSENT]:
                        seen.add('front')
                    if fam == 'row' and ng > 2 * WAVE and not p[WAVE:2 * WAVE].any() and p[WAVE - 1] and p[2 * WAVE]:
                        seen.add('row')
                    if fam == 'every2' and ng >= 63:
                        seen.add('every2')
                    if fam == 'last' and ng >= 2 and p[-1] and not p[:-1].any():
                        seen.add('last')
                # the absences differ per species: a valid gate's rank differs from its gate on both sides of gates 64 and 128
                for j, h in enumerate(c.species):
                    p = pres[h][r, 0]
                    off = p & (np.cumsum(p) - 1 != np.arange(ng))
                    for edge in (WAVE, 2 * WAVE):
                        if ng >= edge + 16 and off[edge - 16:edge].sum() >= 5 and off[edge:edge + 16].sum() >= 5:
                            seen.add(('rank', edge, c.family(r, j)))
    need = {('elevation', e) for e in ELEVATIONS} | {'wgate_zero', 'has_melting_false', 'has_melting_false_on_one_sub_beam', 'rho0_nan',
                                                      'mask_gates', 'zero_q_gates', 'empty', 'all', 'subsets', 'packed_index_differs', 'front',
                                                      'row', 'every2', 'last', 'top'}
    if need - seen:
        bad.append('never staged: %s' % sorted(map(str, need - seen)))
    for edge in (WAVE, 2 * WAVE):
        fams = {k[2] for k in seen if isinstance(k, tuple) and k[0] == 'rank' and k[1] == edge}
        if len(fams) < 2:
            bad.append('rank != gate on both sides of gate %d in fewer than two families: %s' % (edge, sorted(fams)))
    return bad
