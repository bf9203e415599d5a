"""Inputs and a plain restatement for the range scans (scan_lds_wave_exact / scan_lds_sequential, cosmo_pol_amd/csrc/cpol_final.inl,
as they run inside k_final<256>, k_final<512>, k_scan_rays and k_gate1_ray_scan).

PHIDP comes from nan_cumsum(2 KDP), the attenuated ZDR from two nan_cumprods of the per-gate attenuation factors; both are strictly
sequential float32 scans whose order is part of the numerical contract.  What decides whether a kernel keeps it is the NUMBER OF GATES
(rows of 64 lanes, the carry from lane 63 into the next row, the kernels' own thresholds at 256 and 512 gates, the most gates the
library takes) and WHAT THE OPERANDS ARE at the row boundaries (a data-free gate's 0 / 1, signed zeros, subnormals, inf, NaN).  Here are
  * GATE_COUNTS, with N_MAX read from the header the host's own check uses;
  * hook_rows(n, mul): the operand rows of the test hook cpol_debug_scan, each a family built from its name and n;
  * scan_definition(x, mul): the scan by its definition, a float32 loop;
  * SweepCase / make_columns(case): the dict RadarOperator.simulate_columns takes (rain, snow, graupel, 1-moment, no melting, attenuation
    on), every ray one family of data-free gates; oracle_subbeams(case, ray) for the oracle;
  * restate(fields, fh, fv, radial_res): PHIDP and ZDR from a run's own per-gate outputs, in the statements of
    oracle/cosmo_pol_oracle/scatter.py:210-216 and of the kernels' last loop;
  * the coverage the lists must have (hook_coverage_failures, sweep_coverage_failures).
tests/test_scans_cpu.py pins the definition to NumPy and the oracle and asserts the coverage; tests/test_gpu_scans.py pins the device."""
import functools
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def max_gates():
    """CPOL_MAX_GATES of include/cosmo_pol_amd.h: the constant run_sequence compares n_gates with."""
    text = open(os.path.join(ROOT, 'include', 'cosmo_pol_amd.h')).read()
    m = re.findall(r'^#define\s+CPOL_MAX_GATES\s+(\d+)\b', text, flags=re.M)
    assert len(m) == 1, m
    return int(m[0])


N_MAX = max_gates()
GATE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, N_MAX)
ROW = 64                                                 # gates of a row of scan_lds_wave_exact (lanes of a wavefront)
BOUNDARY_GATES = (63, 64, 127, 128)
TINY = np.float32(1.401298464324817e-45)                 # the smallest subnormal float32
MIN_NORMAL = np.float32(1.1754943508222875e-38)

# ------------------------------------------------------------------------------------------------------------ the test hook's rows
ONLY = ('only_first', 'only_last') + tuple('only_%d' % g for g in BOUNDARY_GATES)
SUM_FAMILIES = ('decades', 'neg_zeros', 'mixed_zeros', 'lead_neg_zero', 'inf_mid', 'ninf_mid', 'inf_both', 'nan_mid', 'subnormal',
                'identity') + ONLY
MUL_FAMILIES = ('near_one', 'to_zero', 'sticks', 'overflow', 'decades', 'inf_mid', 'nan_mid', 'zero_then_inf', 'subnormal',
                'identity') + ONLY


def families(mul):
    return MUL_FAMILIES if mul else SUM_FAMILIES


def _only_position(family, n):
    """The gate of an 'only_*' row (None: the row is too short to have it)."""
    g = {'only_first': 0, 'only_last': n - 1}.get(family)
    if g is None:
        g = int(family[5:])
    return g if g < n else None


def hook_row(family, n, mul):
    """One operand row, float32 [n], from the family's name, n and the operation alone."""
    rng = np.random.default_rng(zlib.crc32(('%s/%d/%d' % (family, n, int(mul))).encode()))
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    mid = n // 2
    with np.errstate(over='ignore', under='ignore'):
        if family in ONLY:
            # every operand the identity a data-free gate contributes (0 for the sum, 1 for the product) but one
            x = np.full(n, 1.0 if mul else 0.0)
            g = _only_position(family, n)
            if g is not None:
                x[g] = 0.37 if mul else 1.2345
        elif family == 'identity':
            x = np.full(n, 1.0 if mul else 0.0)
        elif family == 'decades':
            # magnitudes over 12 decades, both signs: a sum in another order differs in many bits
            x = sign * 10.0 ** (rng.uniform(-3.0, 3.0, n) if mul else rng.uniform(-6.0, 6.0, n))
        elif family == 'inf_mid':
            x = rng.uniform(0.9, 1.0, n) if mul else sign * 10.0 ** rng.uniform(-6.0, 6.0, n)
            x[mid] = np.inf
        elif family == 'nan_mid':
            x = rng.uniform(0.9, 1.0, n) if mul else sign * 10.0 ** rng.uniform(-6.0, 6.0, n)
            x[mid] = np.nan
        elif not mul and family == 'neg_zeros':
            x = np.full(n, -0.0)
        elif not mul and family == 'mixed_zeros':
            x = sign * 0.0
        elif not mul and family == 'lead_neg_zero':
            x = sign * 10.0 ** rng.uniform(-6.0, 6.0, n)
            x[0] = -0.0
        elif not mul and family == 'ninf_mid':
            x = sign * 10.0 ** rng.uniform(-6.0, 6.0, n)
            x[mid] = -np.inf
        elif not mul and family == 'inf_both':           # inf, later -inf: NaN from there on
            x = sign * 10.0 ** rng.uniform(-6.0, 6.0, n)
            x[n // 3] = np.inf
            x[(2 * n) // 3] = -np.inf
        elif not mul and family == 'subnormal':          # every operand and every partial sum below the smallest normal number
            x = sign * rng.integers(1, 1 << 9, n) * float(TINY)
        elif mul and family == 'near_one':
            x = 1.0 - rng.uniform(0.0, 0.1, n)           # (0.9, 1]
        elif mul and family == 'to_zero':                # crosses the subnormal range (from gate 95) and reaches exact zero (gate 113)
            x = np.full(n, 0.4)
        elif mul and family == 'sticks':                 # 0.9 x 4 of the smallest subnormal rounds back to 4: never zero (from gate ~970)
            x = np.full(n, 0.9)
        elif mul and family == 'overflow':               # inf from gate 81 on
            x = np.full(n, 3.0)
        elif mul and family == 'zero_then_inf':          # 0, later 0 x inf = NaN
            x = 1.0 - rng.uniform(0.0, 0.1, n)
            x[n // 3] = 0.0
            x[(2 * n) // 3] = np.inf
        elif mul and family == 'subnormal':
            # a cycle whose running product passes 1e30, 1e-10 (by a SUBNORMAL operand), 1e-43 (a subnormal product), 1e-10, 1
            cyc = np.array([1e30, 1e-40, 1e-33, 1e33, 1e10])
            x = cyc[np.arange(n) % 5] * rng.uniform(0.9, 1.1, n)
        else:
            raise ValueError((family, mul))
        return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def hook_rows(n, mul):
    """-> float32 [n_families, n] (read-only), one row per family of families(mul), in that order."""
    x = np.stack([hook_row(f, n, mul) for f in families(mul)])
    x.setflags(write=False)
    return x


def scan_definition(x, mul):
    """The scan by its definition along the last axis: the first element as it is, then c = float32(c op x[i]), one element after
    the other (np.cumsum's / np.cumprod's order)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[-1] >= 1
    out = np.empty_like(x)
    c = x[..., 0].copy()
    out[..., 0] = c
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for i in range(1, x.shape[-1]):
            c = (c * x[..., i] if mul else c + x[..., i]).astype(np.float32)
            out[..., i] = c
    return out


def same_bits(a, b):
    """Equal bits where neither is NaN, NaN at the same places (a NaN's payload does not count)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(u), b[~nb].view(u)))


def where_differs(a, b):
    d = ~((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b)))
    w = np.argwhere(d)
    if not len(w):
        return 'no difference'
    return '%d of %d differ, first at %s: %r against %r' % (len(w), a.size, w[0].tolist(), a[tuple(w[0])], b[tuple(w[0])])


def hook_coverage_failures():
    """What the hook's rows must hold, from the rows and the definition alone."""
    bad = []
    if len(GATE_COUNTS) != 21 or GATE_COUNTS[-1] != N_MAX or 3 * 4 * N_MAX > 65536 or 3 * 4 * (N_MAX + 8) <= 65536:
        bad.append('GATE_COUNTS / N_MAX: %r' % (GATE_COUNTS,))
    for n in (ROW, 2 * ROW, 256, 512, 768, 1024):       # a full last row, and one gate to either side
        if not all(k in GATE_COUNTS for k in (n - 1, n, n + 1)):
            bad.append('no count at %d - 1, %d, %d + 1' % (n, n, n))
    seen = set()
    for n in GATE_COUNTS:
        for mul in (False, True):
            x = hook_rows(n, mul)
            y = scan_definition(x, mul)
            row = dict(zip(families(mul), range(len(x))))
            for f in families(mul):
                xi, yi = x[row[f]], y[row[f]]
                if f in ONLY:
                    g = _only_position(f, n)
                    ident = np.float32(1.0 if mul else 0.0)
                    if g is not None:
                        if not ((np.delete(xi, g) == ident).all() and xi[g] != ident):
                            bad.append('%s at %d gates is not one operand among identities' % (f, n))
                        seen.add((f, mul))
                if f == 'decades' and n >= 63 and not mul:
                    mag = np.log10(np.abs(xi[xi != 0]))
                    if mag.max() - mag.min() < 10 or not (xi < 0).any() or not (xi > 0).any():
                        bad.append('decades at %d gates: %.1f decades' % (n, mag.max() - mag.min()))
                    # (a sum in another order -- pairwise, as a tree scan would form it -- differs in many bits)
                    tree = np.cumsum(xi.astype(np.float64)).astype(np.float32)
                    if (tree != yi).mean() < 0.2:
                        bad.append('decades at %d gates: a float64 scan gives the same bits at %d %% of the gates' % (n, 100 * (tree == yi).mean()))
                    seen.add('decades')
                if f in ('inf_mid', 'ninf_mid', 'inf_both', 'nan_mid', 'zero_then_inf') and n >= 3:
                    special = ~np.isfinite(xi)
                    if not special.any() or (f != 'nan_mid' and special[0]):
                        bad.append('%s at %d gates holds no special value behind gate 0' % (f, n))
                    if f in ('inf_both', 'zero_then_inf', 'nan_mid') and not (np.isnan(yi[-1]) and not np.isnan(yi[0])):
                        bad.append('%s at %d gates does not end in NaN' % (f, n))
                    if f in ('inf_both', 'zero_then_inf', 'nan_mid'):
                        seen.add('nan')
                if f == 'subnormal' and n >= 5:
                    sub_x = (np.abs(xi) < MIN_NORMAL) & (xi != 0)
                    sub_y = (np.abs(yi) < MIN_NORMAL) & (yi != 0)
                    if not sub_x.any() or not sub_y.any():
                        bad.append('subnormal (mul %d) at %d gates: %d subnormal operands, %d subnormal results' % (mul, n, sub_x.sum(), sub_y.sum()))
                    seen.add(('subnormal', mul))
                if f == 'neg_zeros' and not (np.signbit(yi).all() and (yi == 0).all()):
                    bad.append('neg_zeros at %d gates does not stay -0.0' % n)
                if f == 'mixed_zeros' and n >= 63 and not (np.signbit(xi).any() and not np.signbit(xi).all() and (yi == 0).all()):
                    bad.append('mixed_zeros at %d gates' % n)
                if f == 'lead_neg_zero' and n >= 2 and not (np.signbit(yi[0]) and yi[0] == 0 and yi[1] == xi[1]):
                    bad.append('lead_neg_zero at %d gates' % n)
                if mul and f == 'near_one' and not ((xi > 0.9) & (xi <= 1.0)).all():
                    bad.append('near_one at %d gates leaves (0.9, 1]' % n)
                if mul and f == 'to_zero' and n >= 127:
                    sub = (yi < MIN_NORMAL) & (yi > 0)
                    if not (sub.any() and (yi == 0).any() and yi[0] >= MIN_NORMAL and np.flatnonzero(yi == 0)[0] > np.flatnonzero(sub)[-1]):
                        bad.append('to_zero at %d gates does not cross the subnormals and reach zero' % n)
                    seen.add('to_zero')
                if mul and f == 'sticks' and n >= 1023:
                    if not (0 < yi[-1] <= 4 * TINY and (yi == yi[-1]).sum() > 20 and (yi > 0).all()):
                        bad.append('sticks at %d gates does not stick in the subnormals' % n)
                    seen.add('sticks')
                if mul and f == 'overflow' and n >= 127:
                    if not (np.isinf(yi[-1]) and np.isfinite(yi[0])):
                        bad.append('overflow at %d gates' % n)
                    seen.add('overflow')
    need = {(f, m) for f in ONLY for m in (False, True)} | {'decades', 'nan', ('subnormal', False), ('subnormal', True), 'to_zero', 'sticks',
                                                             'overflow'}
    if need - seen:
        bad.append('never staged: %s' % sorted(map(str, need - seen)))
    return bad


# ------------------------------------------------------------------------------------------------------------------ the sweep cases
SPECIES = ('R', 'S', 'G')
Q_OF = {'R': 'QR_v', 'S': 'QS_v', 'G': 'QG_v'}
VARS = ('U', 'V', 'W', 'QR_v', 'QS_v', 'QG_v', 'QI_v', 'RHO', 'T')
RADIAL_RES = 600                                         # radial_resolution of the configuration (an int: the configuration's range check is type-strict)
# every ray one family.  `_q`: the gates are data-free because every mass density is zero; `_mask`: because the sub-beam left the
# model domain there (mask -1 below the topography / +1 above the top, every model value NaN, as the interpolation leaves them)
RAY_FAMILIES = ('precip', 'gates_q', 'gates_mask', 'row_q', 'row_mask', 'alt_q', 'alt_mask', 'empty', 'strong', 'faint')
STRONG_FROM = 63                                         # gate counts from which the strong-attenuation ray can meet its condition
STRONG_LEAD = 4                                          # its first gates hold moderate rain (normal running products)


def config_overrides(sensitivity=None):
    """Rain, snow and graupel of the 1-moment scheme without melting and ice crystals, attenuation on, Doppler scheme 1: the radial
    case c4_7x7 (oracle/gen_golden.py) without its melting species.  Range-dependent sensitivity (10 dBZ at 10 km) unless given."""
    import _cases
    over = _cases.gen_golden.radial_case_inputs('c4_7x7')[0]
    over = {k: dict(v) for k, v in over.items()}
    over['microphysics'].update(with_melting=0, with_ice_crystals=0, with_attenuation=1)
    over['doppler']['scheme'] = 1
    over['radar']['radial_resolution'] = RADIAL_RES
    over['radar']['sensitivity'] = [10, 10000] if sensitivity is None else sensitivity
    return over


class SweepCase(object):
    """n_gates gates, n_sub sub-beams, n_rays rays: ray r is of family RAY_FAMILIES[r mod 10]."""

    def __init__(self, n_gates, n_sub=1, n_rays=len(RAY_FAMILIES)):
        self.n_gates, self.n_sub, self.n_rays = n_gates, n_sub, n_rays
        self.name = 'g%d_s%d_r%d' % (n_gates, n_sub, n_rays)

    def family(self, ray):
        return RAY_FAMILIES[ray % len(RAY_FAMILIES)]

    def rays_of(self, family):
        return [r for r in range(self.n_rays) if self.family(r) == family]

    def __repr__(self):
        return self.name

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self.name == other.name


CASES_1 = tuple(SweepCase(n) for n in GATE_COUNTS)                   # one sub-beam: every single-beam launch form
CASES_4 = tuple(SweepCase(n, n_sub=4) for n in GATE_COUNTS)          # four sub-beams: the general sequence
# k_final<256> beyond 256 gates needs more than 256 rays (with fewer the host picks k_final<512> there)
MANY_RAYS = 257
CASES_MANY_1 = tuple(SweepCase(n, n_rays=MANY_RAYS) for n in (257, 513, 1025))
CASES_MANY_4 = tuple(SweepCase(n, n_sub=4, n_rays=MANY_RAYS) for n in (257, 513, 1025))
ORACLE_COUNTS = (64, 513, 1025, N_MAX)


def data_free(family, n_gates):
    """bool [n_gates]: the gates of a ray of `family` that hold no data."""
    g = np.arange(n_gates)
    base = family.rsplit('_', 1)[0]
    if base == 'gates':                                  # gate 0, the last gate and both sides of the first two row boundaries
        return np.isin(g, (0, n_gates - 1) + BOUNDARY_GATES)
    if base == 'row':                                    # one whole row of the wavefront form
        return (g >= ROW) & (g < 2 * ROW)
    if base == 'alt':
        return g % 2 == 1
    if family == 'empty':
        return np.ones(n_gates, dtype=bool)
    return np.zeros(n_gates, dtype=bool)


def sub_weights(n_sub):
    s = np.arange(n_sub)
    return (1.0 + 0.4 * ((7 * s) % 131) / 131.0) / n_sub


@functools.lru_cache(maxsize=None)
def make_columns(case):
    """The columns of `case` (read-only arrays; computed once per case and shared)."""
    nr, ns, ng = case.n_rays, case.n_sub, case.n_gates
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    shape = (nr, ns, ng)
    cols = {}
    cols['U'] = (20.0 * (1.0 + 0.1 * rng.random(shape))).astype(np.float32)
    cols['V'] = (-15.0 * (1.0 + 0.1 * rng.random(shape)) + 3.0).astype(np.float32)
    cols['W'] = (2.0 * rng.random(shape)).astype(np.float32)
    cols['RHO'] = (0.6 + 0.6 * rng.random((nr, 1, ng)) + 0.01 * rng.random(shape)).astype(np.float32)
    cols['T'] = (215.0 + 75.0 * rng.random((nr, 1, ng)) + rng.uniform(-1.0, 1.0, shape)).astype(np.float32)
    el_ray = rng.uniform(0.3, 8.0, (nr, 1, 1))
    el_sub = rng.uniform(-0.7, 0.7, (1, ns, 1)) if ns > 1 else np.zeros((1, 1, 1))
    elev = np.maximum(el_ray + el_sub + 4e-4 * np.arange(ng)[None, None, :], 0.05)
    cols['elev'] = elev.astype(np.float32)
    cols['quad_pts'] = np.ascontiguousarray(np.stack(
        [np.broadcast_to(1.3 * np.arange(nr)[:, None] + (rng.uniform(-0.7, 0.7, (1, ns)) if ns > 1 else 0.0), (nr, ns)),
         np.broadcast_to((el_ray + el_sub)[:, :, 0], (nr, ns))], axis=-1))
    cols['quad_weights'] = sub_weights(ns)
    mask = np.zeros(shape, dtype=np.int8)
    for h in SPECIES:
        # log-uniform over three decades along the ray, within a factor of 2 across the sub-beams
        cols[Q_OF[h]] = (10.0 ** rng.uniform(-6.0, -3.0, (nr, 1, ng)) * rng.uniform(1.0, 2.0, shape)).astype(np.float32)
    cols['QI_v'] = np.zeros(shape, dtype=np.float32)
    for r in range(nr):
        fam = case.family(r)
        if fam == 'strong':
            # rain alone, moderate at first, then so much that a gate's two-way factors are below 0.1: the running products cross the
            # subnormal range within a few gates and reach zero (tests/test_scans_cpu.py asserts that from the oracle)
            cols['QS_v'][r] = 0
            cols['QG_v'][r] = 0
            cols['QR_v'][r] = (12.0 * rng.uniform(1.0, 1.2, (ns, ng))).astype(np.float32)
            cols['QR_v'][r, :, :STRONG_LEAD] = (1e-3 * rng.uniform(1.0, 2.0, (ns, min(ng, STRONG_LEAD)))).astype(np.float32)
            cols['T'][r] = (283.0 + 4.0 * rng.random((ns, ng))).astype(np.float32)
        elif fam == 'faint':
            # below the sensitivity from the second gate on
            for h in SPECIES:
                cols[Q_OF[h]][r] = (cols[Q_OF[h]][r] * 1e-4).astype(np.float32)
        free = data_free(fam, ng)
        if fam.endswith('_mask'):
            mask[r][:, free] = np.where(np.arange(int(free.sum())) % 2 == 0, 1, -1).astype(np.int8)      # (both codes, in turn)
            for k in VARS:
                cols[k][r][:, free] = np.nan
        elif free.any():
            for h in SPECIES:
                cols[Q_OF[h]][r][:, free] = 0
    cols['mask'] = mask
    for a in cols.values():
        a.setflags(write=False)
    return cols


def oracle_subbeams(case, ray):
    """The oracle's sub-radials of one ray of the columns (fresh arrays: the oracle edits them in place)."""
    from cosmo_pol_oracle.beam import SubBeam
    cols = make_columns(case)
    ng = case.n_gates
    subs = []
    for s in range(case.n_sub):
        values = {k: np.array(cols[k][ray, s], dtype=np.float32) for k in VARS}
        subs.append(SubBeam(values, cols['mask'][ray, s].astype(np.float64), np.zeros(ng), np.zeros(ng),
                            float(RADIAL_RES) * (0.5 + np.arange(ng)), np.zeros(ng), elev=np.array(cols['elev'][ray, s], dtype=np.float32),
                            quad_pt=[float(x) for x in cols['quad_pts'][ray, s]], quad_weight=np.float64(cols['quad_weights'][s])))
    return subs


def factor_exponents(att, radial_res):
    """-0.1f * ATT * res_km in float32, as gate_finish forms it (and NumPy: -0.1 * AV * (radial_res / 1000.) on a float32 array)."""
    att = np.asarray(att)
    assert att.dtype == np.float32
    return np.float32(-0.1) * att * np.float32(radial_res / 1000.)


def numpy_factors(att, radial_res):
    """The per-gate two-way attenuation factors in the reference's statement (float32 power)."""
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        f = 10 ** (-0.1 * np.asarray(att) * (radial_res / 1000.))
    assert f.dtype == np.float32
    return f


def restate(fields, fh, fv, radial_res, scan=scan_definition):
    """(PHIDP, ZDR) from a run's own per-gate outputs `fields` (KDP, DELTA_HV, ZH, ZV: float32 [..., n_gates]) and per-gate factors
    fh, fv (float32, NaN where the gate holds no data):
        k2 = float32(2) * KDP, NaN -> 0;  PHIDP = cumsum(k2) * float32(res) / float32(1000) + DELTA_HV
        ZDR = (ZH * cumprod(fh)) / (ZV * cumprod(fv)), NaN factors -> 1
    every statement in float32."""
    for k in ('KDP', 'DELTA_HV', 'ZH', 'ZV'):
        assert fields[k].dtype == np.float32, k
    assert fh.dtype == np.float32 and fv.dtype == np.float32
    with np.errstate(over='ignore', under='ignore', invalid='ignore', divide='ignore'):
        k2 = np.float32(2) * fields['KDP']
        k2 = np.where(np.isnan(k2), np.float32(0), k2)
        phidp = scan(k2, False) * np.float32(radial_res) / np.float32(1000) + fields['DELTA_HV']
        ph = scan(np.where(np.isnan(fh), np.float32(1), fh), True)
        pv = scan(np.where(np.isnan(fv), np.float32(1), fv), True)
        zdr = (fields['ZH'] * ph) / (fields['ZV'] * pv)
    assert phidp.dtype == np.float32 and zdr.dtype == np.float32
    return phidp, zdr


def strong_condition(fh, fv):
    """What the strong-attenuation ray must show, from its per-gate factors (NaN -> 1) by the definition: for both products at least
    one gate with a subnormal running product, at least one where it is exactly zero, at least one normal gate before them.
    -> list of what is missing."""
    bad = []
    for name, f in (('H', fh), ('V', fv)):
        p = scan_definition(np.where(np.isnan(f), np.float32(1), f).astype(np.float32), True)
        sub = (p > 0) & (p < MIN_NORMAL)
        zero = p == 0
        if not sub.any():
            bad.append('%s: no subnormal running product' % name)
        if not zero.any():
            bad.append('%s: the running product never reaches zero' % name)
        if sub.any() and zero.any() and not (p[:min(np.flatnonzero(sub)[0], np.flatnonzero(zero)[0])] >= MIN_NORMAL).any():
            bad.append('%s: no normal gate before them' % name)
    return bad


def sweep_coverage_failures():
    """What the sweep cases must hold, from the columns alone."""
    bad = []
    if tuple(c.n_gates for c in CASES_1) != GATE_COUNTS or tuple(c.n_gates for c in CASES_4) != GATE_COUNTS:
        bad.append('the cases do not run every gate count')
    if any(c.n_rays <= 256 for c in CASES_MANY_1 + CASES_MANY_4) or set(c.n_gates for c in CASES_MANY_1) != {257, 513, 1025}:
        bad.append('k_final<256> beyond 256 gates: 257 rays at 257, 513 and 1025 gates')
    seen = set()
    for case in CASES_1 + CASES_4 + CASES_MANY_1[:1]:
        cols = make_columns(case)
        ng = case.n_gates
        if set(case.family(r) for r in range(case.n_rays)) != set(RAY_FAMILIES):
            bad.append('%s: not every ray family' % case.name)
        q = sum(np.nan_to_num(cols[Q_OF[h]]) for h in SPECIES)
        for r in range(case.n_rays):
            fam = case.family(r)
            free = data_free(fam, ng)
            has = (q[r] > 0)
            if not (has == ~free[None, :]).all():
                bad.append('%s ray %d (%s): the gates with a positive mass density are not the family\'s' % (case.name, r, fam))
            by_mask = (cols['mask'][r] != 0)
            if fam.endswith('_mask'):
                if not (by_mask == free[None, :]).all() or not np.isnan(cols['T'][r][:, free]).all() or \
                        (ng >= 6 and set(np.unique(cols['mask'][r])) != {-1, 0, 1} and free.sum() >= 2):
                    bad.append('%s ray %d (%s): mask codes' % (case.name, r, fam))
            elif by_mask.any() or np.isnan(cols['T'][r]).any():
                bad.append('%s ray %d (%s): mask codes / NaN outside the mask families' % (case.name, r, fam))
            if fam.startswith('gates_'):
                for g in (0, ng - 1) + BOUNDARY_GATES:
                    if g < ng:
                        seen.add((fam, 'first' if g == 0 else g if g in BOUNDARY_GATES and g != ng - 1 else 'last'))
                        if g in BOUNDARY_GATES:
                            seen.add((fam, g))
            if fam.startswith('row_') and ng > 2 * ROW and free[ROW:2 * ROW].all() and not free[ROW - 1] and not free[2 * ROW]:
                seen.add((fam, 'row'))
            if fam.startswith('alt_') and ng >= 3:
                seen.add((fam, 'alt'))
            if fam == 'empty':
                seen.add('empty')
    need = {(f, p) for f in ('gates_q', 'gates_mask') for p in ('first', 'last') + BOUNDARY_GATES} | \
           {('row_q', 'row'), ('row_mask', 'row'), ('alt_q', 'alt'), ('alt_mask', 'alt'), 'empty'}
    if need - seen:
        bad.append('never staged: %s' % sorted(map(str, need - seen)))
    return bad
