"""Inputs and plain restatements for the radial velocity of Doppler scheme 1 (k_ice_first, subbeam_proj / proj_from_moments,
k_rvel_terms and the accumulation and aliasing of gate_finish, cosmo_pol_amd/csrc/cpol_final.inl).

What decides whether these kernels are right is the NUMBER OF GATES (k_ice_first: lane l of one wavefront adds gates l, l + 64, ...
and a shuffle tree folds the 64 lane sums; the total goes to ONE gate), the NUMBER OF SUB-BEAMS (gate_finish adds the terms in
groups of CPOL_FINAL_SBATCH = 7 plus a tail; below 4 sub-beams it evaluates them in place), WHERE THE ICE IS along a sub-beam and
which sub-beams drop out of a gate (a NaN term neither adds to the sum nor to the weight).  Here are
  * SETS: four species sets under Doppler scheme 1 -- R S G; with 1-moment ice; the melting set R S G mS mG I; the 2-moment
    scheme, whose ice goes through the numeric integrate_V;
  * Case / CASES / make_columns(case): the dict RadarOperator.simulate_columns takes.  Every ray is of one ICE KIND (where the ice
    is) and one DROP KIND (which sub-beam leaves which gates, by mask codes or by NaN winds); the winds differ by metres per second
    between the sub-beams (tests/_subsum.py), so a lost sub-beam moves RVEL by far more than any tolerance;
  * presence(case): which species is valid where, from the columns alone;
  * wave_sum / ice_first: k_ice_first's order; subbeam_proj: the term of one sub-beam; accumulate: the sequential NaN-skipping sum
    and its division by the weight of the non-NaN terms; alias: the folding;
  * oracle_ray: scatter.radar_observables on one ray, with the per-sub-beam terms and the per-species sums it formed on the way;
  * coverage_failures(): what the case list must hold.
tests/test_rvel_cases_cpu.py states the conditions on the oracle alone; tests/test_gpu_rvel.py pins the device."""
import contextlib
import copy
import functools
import zlib

import numpy as np

import _cases
import _scans

N_MAX = _scans.N_MAX                                     # CPOL_MAX_GATES
RADIAL_RES = 300                                         # (an int: the configuration's range check is type-strict)
WAVE = 64                                                # lanes of k_ice_first's wavefront
SBATCH = 7                                               # CPOL_FINAL_SBATCH
NO_GATE = 0x7fffffff                                     # ice_first.first_gate of a sub-beam without valid ice
ATOL = 2e-4                                              # m/s: the suite's figure for RVEL against the oracle
# the worst relative deviation of the float64 oracle's integrate_V from the same formulas in np.longdouble (measured by
# tests/test_rvel_cases_cpu.py, which asserts that it is not exceeded): 1.3e-15 over the gamma species and ice; 1.8e-14 over the
# melting species, whose number density holds the finite difference (D_r(D + 0.01) - D_r(D)) / 0.01.  The device is allowed 8
# times the figure of the species' kind (one figure for all, the larger, would be looser for the gamma species and ice)
ORACLE_WORST = 1.3e-15
ORACLE_WORST_MELTING = 1.8e-14
ORACLE_RTOL = 8 * ORACLE_WORST


def oracle_rtol(h):
    return 8 * (ORACLE_WORST_MELTING if h in MELTING else ORACLE_WORST)

# species set -> the radial case of oracle/gen_golden.py whose configuration it takes (Doppler scheme 1 throughout)
SETS = {'rsg': 'c2_rsg', 'rsgi': 'd3_1mom_ice_sub', 'melt': 'c3_melt_ice', '2mom': 'c5_2mom'}
MELTING = ('mS', 'mG')
ICE = 'I'
Q_RANGE = {'QR_v': (1.0e-6, 2.0e-3), 'QS_v': (1.0e-6, 9.1e-4), 'QG_v': (1.0e-6, 6.5e-4), 'QI_v': (1.0e-7, 1.9e-5),
           'QH_v': (3.3e-7, 6.4e-6), 'QmS_v': (4.1e-4, 2.2e-3), 'QmG_v': (1.0e-6, 6.5e-4),
           'QNR_v': (2.7e-2, 1.1e5), 'QNS_v': (2.8, 1.3e3), 'QNG_v': (2.3e-2, 9.2e2), 'QNH_v': (0.12, 3.2), 'QNI_v': (3.4e3, 5.0e5)}

GATE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 257)
SUB_COUNTS = (1, 2, 3, 4, 6, 7, 8, 13, 14, 15, 22, 29)
ELEVATIONS = (3.0, 45.0, 89.5, 100.0, -5.0, 20.0)        # degrees, as they come (100 and -5 are folded by the product: 80 and 5)
# where the ice is on a ray (the same in every sub-beam but for the weights): from gate 0 / 63 / 64 / 65 on, at the last gate
# alone, at one gate in the first chunk alone, only beyond gate 64 and thinly, nowhere
ICE_KINDS = ('from0', 'from63', 'from64', 'from65', 'last', 'one', 'far', 'none')
ONE_GATE = 5
FAR_FROM = 70
# which sub-beam leaves which gates: 'mask' -- mask codes with NaN values (the sub-beam left the model domain: no species, no
# wind); 'wind' -- NaN winds alone (the species are there, the term is NaN); 'none'
DROP_KINDS = ('mask', 'wind', 'none')
EMPTY_EVERY, EMPTY_AT = 11, 4                            # gates g % 11 == 4 hold no hydrometeor at all, on every ray


@functools.lru_cache(maxsize=None)
def base_overrides(sset):
    over = _cases.gen_golden.radial_case_inputs(SETS[sset])[0]
    return {k: dict(v) for k, v in over.items()}


def config_overrides(sset, nyquist_file=None):
    """The set's radial case with Doppler scheme 1 and this radial resolution; `nyquist_file`: radar/nyquist_velocity."""
    over = copy.deepcopy(base_overrides(sset))
    over['radar'].update(radial_resolution=RADIAL_RES)
    over['doppler'] = {'scheme': 1}
    if nyquist_file is not None:
        over['radar']['nyquist_velocity'] = str(nyquist_file)
    return over


@functools.lru_cache(maxsize=None)
def oracle_setup(sset):
    """-> (oracle configuration, {species: oracle table}, the species in slot order)"""
    from cosmo_pol_oracle import config as ocfg
    conf = ocfg.make_config(config_overrides(sset))
    species = tuple(ocfg.hydrometeor_list(conf))
    ol = {h: _cases.as_oracle_lut(_cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme'])) for h in species}
    return conf, ol, species


def variable_names(sset):
    return tuple(_cases.ORDER_2MOM if sset == '2mom' else _cases.ORDER)


def q_name(h):
    return 'Q' + h + '_v'


class Case(object):
    """n_rays rays of n_sub sub-beams of n_gates gates under species set `sset`.  Ray r is of ice kind ICE_KINDS[(r + rot) mod 8],
    of drop kind DROP_KINDS[(r + rot) mod 3] and at elevation ELEVATIONS[r mod 6]; `wgate`: per-gate weights with zeros."""

    def __init__(self, sset, n_gates, n_sub=1, n_rays=3, rot=0, wgate=False):
        self.sset, self.n_gates, self.n_sub, self.n_rays, self.rot, self.wgate = sset, n_gates, n_sub, n_rays, rot, wgate
        self.species = oracle_setup(sset)[2]
        self.melt = sset == 'melt'
        self.name = '%s_g%d_s%d_r%d_p%d%s' % (sset, n_gates, n_sub, n_rays, rot, '_wgate' if wgate else '')

    def ice_kind(self, ray):
        return ICE_KINDS[(ray + self.rot) % len(ICE_KINDS)]

    def drop_kind(self, ray):
        return DROP_KINDS[(ray + self.rot) % len(DROP_KINDS)]

    def elevation(self, ray):
        return ELEVATIONS[ray % len(ELEVATIONS)]

    def has_ice(self):
        return ICE in self.species

    def __repr__(self):
        return self.name

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self.name == other.name


def _case_list():
    c = []
    # every gate count with ice, the sub-beam counts and the species sets in turn; every ice kind at the counts beyond 64 gates
    c.append(Case('rsgi', 1, n_sub=1, n_rays=8, rot=0))
    c.append(Case('2mom', 2, n_sub=2, n_rays=8, rot=3))
    c.append(Case('melt', 63, n_sub=3, n_rays=3, rot=0))
    c.append(Case('rsgi', 64, n_sub=4, n_rays=4, rot=3))
    c.append(Case('2mom', 65, n_sub=1, n_rays=8, rot=0))
    c.append(Case('rsgi', 65, n_sub=7, n_rays=8, rot=1))
    c.append(Case('melt', 127, n_sub=2, n_rays=4, rot=1))
    c.append(Case('rsgi', 128, n_sub=6, n_rays=4, rot=4))
    c.append(Case('2mom', 129, n_sub=8, n_rays=8, rot=2))
    c.append(Case('rsgi', 129, n_sub=1, n_rays=14, rot=5))
    c.append(Case('melt', 257, n_sub=1, n_rays=8, rot=0))
    c.append(Case('rsgi', 257, n_sub=3, n_rays=8, rot=0))
    # the other sub-beam counts: a tail alone, exact groups of seven, groups and a tail
    c.append(Case('rsg', 65, n_sub=13, n_rays=3, rot=0))
    c.append(Case('rsgi', 65, n_sub=14, n_rays=3, rot=1))
    c.append(Case('melt', 17, n_sub=15, n_rays=3, rot=2))
    c.append(Case('rsgi', 66, n_sub=22, n_rays=3, rot=2))
    c.append(Case('2mom', 33, n_sub=29, n_rays=3, rot=5))
    c.append(Case('rsg', 129, n_sub=1, n_rays=6, rot=0))
    c.append(Case('rsg', 130, n_sub=3, n_rays=3, rot=1))                       # (no table-borne Doppler sums: k_final evaluates the table items in place)
    # per-gate weights with zeros: in place (3), a tail alone (6), a group and a tail (8), two groups (14)
    c.append(Case('rsgi', 129, n_sub=3, n_rays=8, rot=0, wgate=True))
    c.append(Case('melt', 65, n_sub=6, n_rays=4, rot=4, wgate=True))
    c.append(Case('2mom', 66, n_sub=8, n_rays=8, rot=0, wgate=True))
    c.append(Case('rsgi', 70, n_sub=14, n_rays=5, rot=1, wgate=True))
    # the most gates: k_ice_first's strided loop at its longest (one ray, ice from gate 64 on)
    c.append(Case('rsgi', N_MAX, n_sub=1, n_rays=1, rot=2))
    return tuple(c)


def sub_weights(n_sub):
    """Distinct and of one magnitude (tests/_subsum.py); one sub-beam: [1.0]."""
    s = np.arange(n_sub)
    return (1.0 + 0.4 * ((7 * s) % 131) / 131.0) / n_sub if n_sub > 1 else np.ones(1)


def ice_pattern(kind, n_gates):
    """bool [n_gates]: the gates that hold ice on a ray of `kind` (before the gates without any hydrometeor are taken out)."""
    g = np.arange(n_gates)
    if kind.startswith('from'):
        return g >= min(int(kind[4:]), n_gates - 1)
    if kind == 'last':
        return g == n_gates - 1
    if kind == 'one':
        return g == min(ONE_GATE, n_gates - 1)
    if kind == 'far':
        return (g >= FAR_FROM) & (g % 3 == 1) if n_gates > FAR_FROM else g == n_gates - 1
    if kind == 'none':
        return np.zeros(n_gates, dtype=bool)
    raise ValueError(kind)


def empty_gates(n_gates):
    """bool [n_gates]: the gates without any hydrometeor (never the gates the ice kinds are about)."""
    g = np.arange(n_gates)
    return (g % EMPTY_EVERY == EMPTY_AT) & (g != n_gates - 1)


def dropped(case, ray):
    """bool [n_sub, n_gates]: where the ray's drop kind takes a sub-beam out of a gate: sub-beam (g // 7) mod n_sub at the gates
    g % 7 == 3 -- with one sub-beam, the gate is left without a term."""
    ns, ng = case.n_sub, case.n_gates
    d = np.zeros((ns, ng), dtype=bool)
    if case.drop_kind(ray) == 'none':
        return d
    g = np.arange(ng)
    at = g % 7 == 3
    d[(g[at] // 7) % ns, g[at]] = True
    return d


def species_pattern(h, j, n_gates):
    """bool [n_gates]: where a species other than ice is planned."""
    g = np.arange(n_gates)
    if n_gates <= 2:
        return np.ones(n_gates, dtype=bool)
    return {0: np.ones(n_gates, dtype=bool), 1: g % 2 == 1, 2: g >= n_gates // 3, 3: g % 3 != 2, 4: g % 5 != 0}[j % 5]


def fold(elev):
    """The in-place fold of doppler_scatter.py:173-176 (quirk Q8)."""
    elev[elev > 90] = 180 - elev[elev > 90]
    elev[elev < 0] = -elev[elev < 0]
    return elev


@functools.lru_cache(maxsize=None)
def make_columns(case):
    """The columns of `case` (read-only arrays; computed once per case and shared)."""
    nr, ns, ng = case.n_rays, case.n_sub, case.n_gates
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    shape = (nr, ns, ng)
    names = variable_names(case.sset)
    s = np.arange(ns)
    sign = np.where(s % 2 == 0, 1.0, -1.0)[None, :, None]
    cols = {}
    # winds differing strongly between sub-beams: a sub-beam lost from the weighted mean moves it by metres per second
    cols['U'] = (20.0 * sign * (1.0 + 0.1 * rng.random(shape))).astype(np.float32)
    cols['V'] = (-15.0 * sign * (1.0 + 0.1 * rng.random(shape)) + 3.0).astype(np.float32)
    cols['W'] = (2.0 * sign * rng.random(shape)).astype(np.float32)
    cols['RHO'] = (0.6 + 0.6 * rng.random((nr, 1, ng)) + 0.01 * rng.random(shape)).astype(np.float32)
    cols['T'] = (215.0 + 75.0 * rng.random((nr, 1, ng)) + rng.uniform(-1.0, 1.0, shape)).astype(np.float32)
    el_ray = np.array([case.elevation(r) for r in range(nr)])[:, None, None]
    el_sub = rng.uniform(-0.7, 0.7, (1, ns, 1)) if ns > 1 else np.zeros((1, 1, 1))
    az_sub = rng.uniform(-0.7, 0.7, (1, ns)) if ns > 1 else np.zeros((1, 1))
    cols['elev'] = (el_ray + el_sub + 0.01 * (np.arange(ng) % 200)[None, None, :]).astype(np.float32)      # (89.5 deg crosses 90 at gate 50)
    cols['quad_pts'] = np.ascontiguousarray(np.stack(
        [np.broadcast_to(37.0 * np.arange(nr)[:, None] + az_sub, (nr, ns)), np.broadcast_to((el_ray + el_sub)[:, :, 0], (nr, ns))], axis=-1))
    for k in names:
        cols.setdefault(k, np.zeros(shape, dtype=np.float32))
    qs = [q_name(h) for h in case.species]
    for k in qs + (['QN' + h + '_v' for h in case.species] if case.sset == '2mom' else []):
        lo, hi = Q_RANGE[k]
        # log-uniform along the ray, within a factor of 2 across the sub-beams
        cols[k] = (np.exp(rng.uniform(np.log(lo), np.log(hi / 2), (nr, 1, ng))) * rng.uniform(1.0, 2.0, shape)).astype(np.float32)
    if case.melt:
        cols['fwet_mS'] = rng.uniform(0.02, 0.98, shape)
        cols['fwet_mG'] = rng.uniform(0.02, 0.98, shape)
        hm = np.ones((nr, ns), dtype=np.int8)
        hm[(np.arange(nr)[:, None] + s[None, :]) % 4 == 1] = 0                  # has_melting False on some sub-beams
        cols['has_melting'] = hm
    empty = empty_gates(ng)
    mask = np.zeros(shape, dtype=np.int8)
    for r in range(nr):
        for j, h in enumerate(case.species):
            p = ice_pattern(case.ice_kind(r), ng) if h == ICE else species_pattern(h, j, ng)
            cols[q_name(h)][r][:, ~(p & ~empty)] = 0
        d = dropped(case, r)
        if case.drop_kind(r) == 'mask':
            code = np.where((np.arange(ng) // 7) % 2 == 0, 1, -1).astype(np.int8)          # (both codes, in turn)
            mask[r][d] = np.broadcast_to(code[None, :], d.shape)[d]
            for k in names + (('QmS_v', 'QmG_v') if case.melt else ()):
                cols[k][r][d] = np.nan
        elif case.drop_kind(r) == 'wind':
            for i, k in enumerate(('U', 'V', 'W')):
                sel = d & ((np.arange(ng) // 7) % 3 == i)[None, :]
                cols[k][r][sel] = np.nan
    cols['mask'] = mask
    if case.wgate:
        w = sub_weights(ns)[None, :, None] * (1.0 + 0.2 * rng.random(shape))
        w[rng.random(shape) < 0.15] = 0.0
        for r in range(nr):
            # sub-beam 0 loses the weight of its first ice gate: the total must move to its next valid gate
            ice = np.flatnonzero(cols[q_name(ICE)][r, 0] > 0) if case.has_ice() else []
            if len(ice) > 1:
                w[r, 0, ice[0]] = 0.0
                w[r, 0, ice[1]] = max(w[r, 0, ice[1]], 0.5 / ns)
            w[r, :, ng // 2] = 0.0 if r % 2 == 0 else w[r, :, ng // 2]          # a gate where every weight is 0
        cols['quad_weights'] = w
    else:
        cols['quad_weights'] = sub_weights(ns)
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


def alone(case, sub):
    """The columns of sub-beam `sub` of the case as a call of its own: the scalar weight 1.0, or -- a case with per-gate weights --
    per-gate weights 1.0 where the case's are > 0 and 0.0 where they are 0 (a zero weight removes the gate's species: the sub-beam
    alone must lose the same gates, and with them the gate its ice total goes to)."""
    cols = make_columns(case)
    out = {}
    for k, a in cols.items():
        if k == 'quad_weights':
            out[k] = (a[:, sub:sub + 1] > 0).astype(np.float64) if case.wgate else np.ones(1)
        elif k in ('quad_pts', 'has_melting') or np.ndim(a) == 3:
            out[k] = np.ascontiguousarray(a[:, sub:sub + 1])
        else:
            out[k] = a
    return out


def weights_of(case, ray):
    """float64 [n_sub, n_gates]: the weight of every term of a ray as gate_finish takes it (sub_w[s], or wgate)."""
    w = make_columns(case)['quad_weights']
    return np.array(w[ray]) if case.wgate else np.repeat(np.asarray(w, dtype=np.float64)[:, None], case.n_gates, axis=1)


# ------------------------------------------------------------------------------------------------------------------- the oracle
def oracle_subbeams(case, ray, subs=None, alone_weights=False):
    """The oracle's sub-radials of one ray of the columns (fresh arrays: the oracle edits them in place).  alone_weights: every
    sub-beam with the weights of alone()."""
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
        if alone_weights:
            qw = (np.array(w[ray, s]) > 0).astype(np.float64) if case.wgate else np.float64(1.0)
        else:
            qw = np.array(w[ray, s]) if case.wgate else np.float64(w[s])
        sb = SubBeam(values, cols['mask'][ray, s].astype(np.float64), np.zeros(ng), np.zeros(ng), float(RADIAL_RES) * (0.5 + np.arange(ng)),
                     np.zeros(ng), elev=np.array(cols['elev'][ray, s], dtype=np.float32), quad_pt=[float(x) for x in cols['quad_pts'][ray, s]],
                     quad_weight=qw)
        if case.melt:
            sb.has_melting = bool(cols['has_melting'][ray, s])
        out.append(sb)
    return out


@contextlib.contextmanager
def _recording(book):
    """scatter.radar_observables with its proj_vel and every species' integrate_V recorded into `book`."""
    from cosmo_pol_oracle import scatter
    own_proj, own_create = scatter.proj_vel, scatter.create_hydrometeor

    def proj_vel(*a):
        p = own_proj(*a)
        book['proj'].append(np.array(p, dtype=np.float64))
        book['sums'].append(book['pending'])             # (what integrate_V returned for this sub-beam, in slot order)
        book['pending'] = []
        return p

    def create(h, scheme):
        obj = own_create(h, scheme)
        inner = obj.integrate_V

        def integrate_V():
            v, n = inner()
            book['pending'].append((h, np.array(v, dtype=np.float64), np.array(n, dtype=np.float64)))
            return v, n
        obj.integrate_V = integrate_V
        return obj
    scatter.proj_vel, scatter.create_hydrometeor = proj_vel, create
    try:
        yield
    finally:
        scatter.proj_vel, scatter.create_hydrometeor = own_proj, own_create


def oracle_ray(case, ray, subs=None, alone_weights=False, nyquist=None):
    """scatter.radar_observables on the sub-beams `subs` (all) of one ray -> dict(RVEL [n_gates], proj [n_sub, n_gates]: the term
    of every sub-beam as the oracle formed it, sums: per sub-beam a list of (species, v, n) as integrate_V returned them -- over the
    species' valid gates; ice: one total)."""
    from cosmo_pol_oracle import scatter
    conf, ol, _ = oracle_setup(case.sset)
    sbs = oracle_subbeams(case, ray, subs=subs, alone_weights=alone_weights)
    book = {'proj': [], 'sums': [], 'pending': []}
    with _recording(book):
        o = scatter.radar_observables(sbs, ol, conf, nyquist=nyquist)
    return {'RVEL': np.asarray(o.values['RVEL'], dtype=np.float64), 'proj': np.stack(book['proj']), 'sums': book['sums']}


# ------------------------------------------------------------------------------------------------------------- k_ice_first, restated
def wave_sum(x, valid):
    """float64 [n_gates], bool [n_gates] -> the sum of the valid entries in the order of k_ice_first's wavefront: lane l adds
    gates l, l + 64, ... in ascending order from +0.0 (an invalid gate is skipped), then for off = 32, 16, ... 1 every lane
    l < off adds lane l + off; lane 0 holds the result."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    lanes = np.zeros(WAVE, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for g0 in range(0, n, WAVE):
            chunk = np.zeros(WAVE, dtype=np.float64)
            ok = np.zeros(WAVE, dtype=bool)
            m = min(WAVE, n - g0)
            chunk[:m], ok[:m] = x[g0:g0 + m], valid[g0:g0 + m]
            lanes = np.where(ok, lanes + chunk, lanes)
        off = WAVE // 2
        while off >= 1:
            lanes[:off] = lanes[:off] + lanes[off:2 * off]
            off //= 2
    return lanes[0]


def ice_first(vn, valid):
    """vn float64 [n_gates, 2] (a species' per-gate sums), valid bool [n_gates] -> (first valid gate or NO_GATE, v, n) of
    k_ice_first."""
    w = np.flatnonzero(valid)
    return (int(w[0]) if len(w) else NO_GATE), wave_sum(vn[:, 0], valid), wave_sum(vn[:, 1], valid)


# ------------------------------------------------------------------------------------------------------------ subbeam_proj, restated
def az_sincos(quad_pts):
    """[..., 2] exactly as simulate_columns forms it."""
    from cosmo_pol_amd import geometry as geo
    az_rad = np.asarray(quad_pts, dtype=np.float64)[..., 0] * geo.DEG
    return np.stack([np.sin(az_rad), np.cos(az_rad)], axis=-1)


def trig32(elev32, nudge=(0, 0)):
    """(cos, sin) of np.deg2rad(float32 folded elevation): the float64 value rounded once to float32, as the device forms it.
    nudge: units in the last place by which to move (cos, sin) -- for the one-ulp rule of the term's comparison."""
    elev32 = np.asarray(elev32)
    assert elev32.dtype == np.float32
    th = elev32 * np.float32(0.017453292)                # np.deg2rad on float32
    assert th.dtype == np.float32
    ct, st = np.cos(th.astype(np.float64)).astype(np.float32), np.sin(th.astype(np.float64)).astype(np.float32)
    for a, k in ((ct, nudge[0]), (st, nudge[1])):
        for _ in range(abs(k)):
            a[...] = np.nextafter(a, np.float32(np.inf if k > 0 else -np.inf))
    return ct, st


def moments(vn, valid, vsrc, first=None):
    """The fall-speed sums (v, nn) of one sub-beam as subbeam_proj forms them: vn float64 [n_hydro, n_gates, 2], valid bool
    [n_hydro, n_gates], vsrc [n_hydro] (1: per gate; 2: the species' total at its first valid gate), first: {slot: (gate, v, n)}
    for the slots with vsrc 2 (default: ice_first of the slot's own vn).  In slot order, a NaN summand skipped."""
    nh, ng = valid.shape
    v, nn = np.zeros(ng), np.zeros(ng)
    for j in range(nh):
        if vsrc[j] == 1:
            vj, nj = vn[j, :, 0], vn[j, :, 1]
        else:
            g0, tv, tn = ice_first(vn[j], valid[j]) if first is None else first[j]
            here = np.arange(ng) == g0
            vj, nj = np.where(here, tv, 0.0), np.where(here, tn, 0.0)
        with np.errstate(invalid='ignore'):
            v = np.where(valid[j] & ~np.isnan(vj), v + vj, v)
            nn = np.where(valid[j] & ~np.isnan(nj), nn + nj, nn)
    return v, nn


def proj_from_moments(v, nn, U, V, W, elev32, sincos, nudge=(0, 0), trig='rounded'):
    """proj_from_moments of cpol_final.inl: (U sin(az) + V cos(az)) ct + (W - v / nn) st in float64, U V W float32 widened, the
    elevation folded (float32) and ct, st of trig32 (trig 'numpy': NumPy's float32 cosine and sine, as the oracle takes them)."""
    e = fold(np.array(elev32, dtype=np.float32))
    if trig == 'numpy':
        th = np.deg2rad(e)
        assert th.dtype == np.float32
        ct, st = np.cos(th), np.sin(th)
    else:
        ct, st = trig32(e, nudge)
    with np.errstate(invalid='ignore', divide='ignore'):
        vh = v / nn
        U, V, W = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (U, V, W))
        return (U * sincos[0] + V * sincos[1]) * ct.astype(np.float64) + (W - vh) * st.astype(np.float64)


def trig32_exact(elev32):
    """(cos, sin) of the same float32 angle evaluated in np.longdouble and rounded once to float32."""
    th = np.asarray(elev32, dtype=np.float32) * np.float32(0.017453292)
    return np.cos(th.astype(np.longdouble)).astype(np.float32), np.sin(th.astype(np.longdouble)).astype(np.float32)


# --------------------------------------------------------------------------------------------- the oracle's sums, item by item
def hydrometeor(case, h):
    """The oracle's hydrometeor object of a species as scatter.radar_observables prepares it."""
    from cosmo_pol_oracle.psd import create_hydrometeor
    conf, ol, _ = oracle_setup(case.sset)
    hyd = create_hydrometeor(h, conf['microphysics']['scheme'])
    hyd.nbins_D = ol[h].value_table.shape[-2]
    d_ax = ol[h].axes[2]
    hyd.d_min = d_ax[:, 0] if h in MELTING else d_ax[0]
    hyd.d_max = d_ax[:, -1] if h in MELTING else d_ax[-1]
    return hyd


def _set_psd(case, hyd, h, values, sel):
    scheme = oracle_setup(case.sset)[0]['microphysics']['scheme']
    T, QM = values['T'], values[q_name(h)]
    if scheme == '1mom':
        if h == 'mG':
            hyd.set_psd(QM[sel], values['fwet_' + h][sel])
        elif h == 'mS':
            hyd.set_psd(T[sel], QM[sel], values['fwet_' + h][sel])
        elif h in ('S', 'I'):
            hyd.set_psd(T[sel], QM[sel])
        else:
            hyd.set_psd(QM[sel])
    else:
        hyd.set_psd(values['QN' + h + '_v'][sel], QM[sel])


def closed_form_longdouble(hyd):
    """integrate_V of a gamma species (hydrometeors.py:178-199) in np.longdouble from the object's lambda and N0."""
    L = np.longdouble
    lam, n0 = L(np.atleast_1d(hyd.lambda_)), L(np.atleast_1d(hyd.N0))
    v = L(hyd.vel_factor) * n0 * L(hyd.alpha) / L(hyd.nu) * lam ** (-(L(hyd.beta) + L(hyd.mu) + 1) / L(hyd.nu))
    if hyd.scheme == '2mom':
        n = L(np.atleast_1d(hyd.ntot))
    else:
        n = L(hyd.ntot_factor) * n0 / L(hyd.nu) * lam ** (-(L(hyd.mu) + 1) / L(hyd.nu))
    return v, n


def ice_sums_longdouble(hyd):
    """IceParticle.integrate_V (hydrometeors.py:1256-1275) with the same float32 diameters and fall speeds, N0 and lambda; the
    number densities, the products and the sums in np.longdouble."""
    L = np.longdouble
    D = np.linspace(hyd.d_min, hyd.d_max, hyd.nbins_D)
    dD = L(D[1] - D[0])
    own = hyd.N0, hyd.lambda_
    hyd.N0, hyd.lambda_ = L(np.atleast_1d(hyd.N0)), L(np.atleast_1d(hyd.lambda_))
    try:
        if hyd.scheme == '1mom':
            N = hyd.get_N(L(D))
        else:                                            # (the float32 powers D^mu and D^nu are data, like alpha D^beta)
            N = hyd.N0[:, None] * L(D ** hyd.mu) * np.exp(-hyd.lambda_[:, None] * L(D ** hyd.nu))
        V = L(hyd.get_V(D))                              # (the float32 power table alpha D^beta is data: the product takes it from the host too)
        assert N.dtype == np.longdouble
        return np.sum(N * V) * dD, np.sum(N) * dD
    finally:
        hyd.N0, hyd.lambda_ = own


def melting_sums_longdouble(hyd):
    """Melting.integrate_V (hydrometeors.py:441-460) on the same float64 diameters with the same PSD parameters (the rain's and the
    solid's lambda and N0, the wet fraction, the mass normalisation), every operation in np.longdouble."""
    from cosmo_pol_oracle.psd import vlinspace
    L = np.longdouble
    D = vlinspace(hyd.d_min, hyd.d_max, hyd.nbins_D)
    dD = L(D[:, 1] - D[:, 0])
    parts = (hyd.rain, hyd.solid)
    own = [(p.lambda_, p.N0) for p in parts], hyd._f_wet, hyd.prop_factor
    for p in parts:
        p.lambda_, p.N0 = L(p.lambda_), (L(p.N0) if not np.isscalar(p.N0) else L(p.N0))
    hyd._f_wet, hyd.prop_factor = L(hyd._f_wet), L(hyd.prop_factor)
    try:
        N, V = hyd.get_N(L(D)), hyd.get_V(L(D))
        assert N.dtype == np.longdouble and V.dtype == np.longdouble
        return np.sum(N * V, axis=1) * dD, np.sum(N, axis=1) * dD
    finally:
        for p, (lam, n0) in zip(parts, own[0]):
            p.lambda_, p.N0 = lam, n0
        hyd._f_wet, hyd.prop_factor = own[1], own[2]


def oracle_moments(case, ray, sub, measure=None):
    """The oracle's own integrate_V of every species of one sub-beam, item by item: -> (v, n) float64 [n_hydro, n_gates], NaN where
    the species is not valid.  Ice: integrate_V restricted to one gate at a time.  measure: a dict that collects, per species, the
    worst relative deviation of these float64 values from the same formulas in np.longdouble (gamma species and ice)."""
    sb = oracle_subbeams(case, ray, subs=[sub])[0]
    fold(sb.elev_profile)
    pres = presence(case)
    ng = case.n_gates
    v, n = np.full((len(case.species), ng), np.nan), np.full((len(case.species), ng), np.nan)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for j, h in enumerate(case.species):
            valid = pres[h][ray, sub]
            if not valid.any():
                continue
            hyd = hydrometeor(case, h)
            if h == ICE:
                for g in np.flatnonzero(valid):
                    _set_psd(case, hyd, h, sb.values, slice(g, g + 1))
                    a, b = hyd.integrate_V()
                    v[j, g], n[j, g] = float(np.ravel(a)[0]), float(np.ravel(b)[0])
                    if measure is not None:
                        la, lb = ice_sums_longdouble(hyd)
                        dev = max(abs(float((v[j, g] - la) / la)), abs(float((n[j, g] - lb) / lb)))
                        measure[h] = max(measure.get(h, 0.0), dev)
            else:
                _set_psd(case, hyd, h, sb.values, valid)
                a, b = hyd.integrate_V()
                v[j, valid], n[j, valid] = a, b
                if measure is not None:
                    la, lb = melting_sums_longdouble(hyd) if h in MELTING else closed_form_longdouble(hyd)
                    dev = max(float(np.max(np.abs((v[j, valid] - la) / la))), float(np.max(np.abs((n[j, valid] - lb) / lb))))
                    measure[h] = max(measure.get(h, 0.0), dev)
    return v, n


def vsrc_of(case):
    """FinalArgs::vsrc under Doppler scheme 1: 2 for ice crystals (1-moment: the ice field; 2-moment: numeric integrate_V)."""
    return [2 if h == ICE else 1 for h in case.species]


# ------------------------------------------------------------------------------------------------------------ gate_finish, restated
def accumulate(terms, weights):
    """terms, weights float64 [n_sub, n_gates] -> RVEL before the folding: rv starts NaN and tw 0.0; per sub-beam in order, where
    the term is not NaN tw += w; rv = (0 if isnan(rv) else rv) + (0 if isnan(term w) else term w); then rv / tw
    (doppler_scatter.py:313-333, 418-420)."""
    terms, weights = np.asarray(terms, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    assert terms.shape == weights.shape and terms.ndim == 2
    rv, tw = np.full(terms.shape[1], np.nan), np.zeros(terms.shape[1])
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for s in range(terms.shape[0]):
            tw = np.where(np.isnan(terms[s]), tw, tw + weights[s])
            y = terms[s] * weights[s]
            rv = np.where(np.isnan(rv), 0.0, rv) + np.where(np.isnan(y), 0.0, y)
        return rv / tw


def alias(rv, nyq):
    """utilities.py:142-156 as gate_finish writes it."""
    with np.errstate(invalid='ignore'):
        theta = (rv + nyq) / (2 * nyq) * np.pi - np.pi / 2.
        return (np.arctan(np.tan(theta)) + np.pi / 2) * (2 * nyq) / np.pi - nyq


def alias_theta(rv, nyq):
    return (rv + nyq) / (2 * nyq) * np.pi - np.pi / 2.


def pole_distance(theta):
    """Distance of theta from the nearest pole of the tangent, pi / 2 + k pi."""
    return np.abs((theta / np.pi - 0.5) - np.round(theta / np.pi - 0.5)) * np.pi


# ------------------------------------------------------------------------------------------------------------------- the coverage
CASES = _case_list()
BY_NAME = {c.name: c for c in CASES}
MULTI = tuple(c for c in CASES if c.n_sub > 1)
TOP = CASES[-1]
# the folding: one case per species set, one, two, seven and eight sub-beams, one with per-gate weights
ALIAS_CASES = tuple(BY_NAME[k] for k in ('rsg_g129_s1_r6_p0', 'melt_g127_s2_r4_p1', 'rsgi_g65_s7_r8_p1', '2mom_g66_s8_r8_p0_wgate'))
# elevation of the row -> Nyquist velocity (m/s): the rows of the radar/nyquist_velocity file, one per elevation of ELEVATIONS
# (the row nearest in elevation to the central sub-beam counts); |RVEL| reaches 25 m/s: dozens of Nyquist intervals at the smallest
NYQUIST_ROWS = ((3.0, 0.7), (45.0, 1.3), (89.5, 2.1), (100.0, 3.3), (-5.0, 0.45), (20.0, 6.0))
POLE_MARGIN = 1e-9


def nyquist_text():
    return 'elevation,azimuth,nyquist\n' + ''.join('%r,0,%r\n' % row for row in NYQUIST_ROWS)


def nyquist_of(case):
    """float64 [n_rays]: the Nyquist velocity of every ray, by the rule of cosmo_pol_amd/nyquist.py on the central sub-beam."""
    qp = make_columns(case)['quad_pts'][:, int(case.n_sub / 2)]
    rows = np.array(NYQUIST_ROWS)
    return np.array([rows[np.argmin(np.abs(rows[:, 0] - el)), 1] for el in qp[:, 1]])


def first_ice_gates(case, cols=None):
    """int [n_rays, n_sub]: the first valid ice gate of every sub-beam (NO_GATE: none), and the number of valid ice gates."""
    p = presence(case, cols)[ICE]
    first = np.where(p.any(axis=2), p.argmax(axis=2), NO_GATE)
    return first, p.sum(axis=2)


def coverage_failures(cases=None):
    """What the case list must hold for the comparisons on the device to mean something, from the columns alone."""
    cases = CASES if cases is None else cases
    bad, seen = [], set()
    gates = {c.n_gates for c in cases}
    if not set(GATE_COUNTS) <= gates or N_MAX not in gates:
        bad.append('gate counts: %s' % sorted((set(GATE_COUNTS) | {N_MAX}) - gates))
    if not set(SUB_COUNTS) <= {c.n_sub for c in cases}:
        bad.append('sub-beam counts: %s' % sorted(set(SUB_COUNTS) - {c.n_sub for c in cases}))
    if {c.sset for c in cases} != set(SETS):
        bad.append('species sets')
    if any(not 3 <= c.n_rays <= 14 for c in cases if c.n_gates != N_MAX):
        bad.append('rays outside 3 ... 14')
    # the sub-beam counts as gate_finish sees them: in place (< 4), a tail alone, exact groups, groups and a tail
    for c in cases:
        n = c.n_sub
        seen.add('inplace' if n < 4 else 'tail_only' if n < SBATCH else 'exact_groups' if n % SBATCH == 0 else 'groups_and_tail')
        if n >= 2 * SBATCH:
            seen.add('two_groups')
    for c in cases:
        cols = make_columns(c)
        pres = presence(c, cols)
        ng, ns = c.n_gates, c.n_sub
        w = cols['quad_weights']
        seen.add(('set', c.sset))
        if ns > 1 and not c.wgate and (len(np.unique(w)) != ns or w.max() > 2 * w.min()):
            bad.append('%s: weights' % c.name)
        if ns > 1:
            # winds that differ by metres per second between neighbouring sub-beams
            with np.errstate(invalid='ignore'):
                du = np.abs(np.diff(cols['U'].astype(np.float64), axis=1))
            if not np.nanmin(du) > 10.0:
                bad.append('%s: winds of neighbouring sub-beams within %g m/s' % (c.name, np.nanmin(du)))
        if c.wgate:
            if np.ndim(w) != 3 or not (w == 0).any():
                bad.append('%s: per-gate weights' % c.name)
            seen.add(('wgate', c.name))
            if (w == 0).all(axis=1).any():
                seen.add('all_weights_zero')
        if c.melt and (cols['has_melting'] == 0).any() and (cols['has_melting'] != 0).any():
            seen.add('has_melting_false')
        anyh = np.zeros((c.n_rays, ns, ng), dtype=bool)
        for h in c.species:
            anyh |= pres[h]
        if c.has_ice():
            first, count = first_ice_gates(c, cols)
            plain = presence(c, cols, weights=False)[ICE]
            for r in range(c.n_rays):
                kind = c.ice_kind(r)
                for s in range(ns):
                    f, n = int(first[r, s]), int(count[r, s])
                    if n == 0:
                        seen.add('no_ice')
                        continue
                    if f in (0, 63, 64, 65) and n > 1 and ng > 66:
                        seen.add(('first', f))
                    if f == ng - 1 and ng > 1:
                        seen.add('first_is_last')
                    if n == 1 and ng > 2:
                        seen.add('one_gate')
                    if f > WAVE and ng > WAVE:
                        seen.add('beyond_64')
                    if n > 1 and f < WAVE <= np.flatnonzero(pres[ICE][r, s])[-1]:
                        seen.add('both_sides_of_64')
                    if c.wgate and plain[r, s].any() and int(plain[r, s].argmax()) < f and w[r, s, int(plain[r, s].argmax())] == 0:
                        seen.add('first_ice_gate_weight_zero')
                if kind == 'none' and count[r].sum() != 0:
                    bad.append('%s ray %d: ice on a ray of kind none' % (c.name, r))
        for r in range(c.n_rays):
            seen.add(('elevation', c.elevation(r)))
            e = cols['elev'][r]
            if np.nanmax(e) > 90:
                seen.add('above_90')
            if np.nanmin(e) < 0:
                seen.add('below_0')
            d = dropped(c, r)
            by_mask = cols['mask'][r] != 0
            with np.errstate(invalid='ignore'):
                nan_wind = np.isnan(cols['U'][r]) | np.isnan(cols['V'][r]) | np.isnan(cols['W'][r])
            if c.drop_kind(r) == 'mask':
                if not np.array_equal(by_mask, d) or not np.isnan(cols['T'][r][d]).all() or anyh[r][d].any():
                    bad.append('%s ray %d: mask codes' % (c.name, r))
                if d.any() and ns > 1 and (d.sum(axis=0) == 1).any():
                    seen.add('mask_drops_one_sub_beam')
                if d.sum() >= 2 and set(np.unique(cols['mask'][r])) == {-1, 0, 1}:
                    seen.add('both_mask_codes')
            elif by_mask.any():
                bad.append('%s ray %d: mask codes outside the mask kind' % (c.name, r))
            if c.drop_kind(r) == 'wind':
                if not np.array_equal(nan_wind, d):
                    bad.append('%s ray %d: NaN winds' % (c.name, r))
                if ns > 1 and (d & anyh[r]).any():
                    seen.add('nan_wind_drops_one_sub_beam')
            e_g = empty_gates(ng)
            if e_g.any():
                if anyh[r][:, e_g].any():
                    bad.append('%s ray %d: a hydrometeor at an empty gate' % (c.name, r))
                if c.drop_kind(r) == 'none':
                    seen.add('empty_gates')
    need = {('elevation', e) for e in ELEVATIONS} | {('set', k) for k in SETS} | {('first', f) for f in (0, 63, 64, 65)} | {
        'inplace', 'tail_only', 'exact_groups', 'groups_and_tail', 'two_groups', 'no_ice', 'first_is_last', 'one_gate', 'beyond_64',
        'both_sides_of_64', 'first_ice_gate_weight_zero', 'all_weights_zero', 'has_melting_false', 'above_90', 'below_0',
        'mask_drops_one_sub_beam', 'both_mask_codes', 'nan_wind_drops_one_sub_beam', 'empty_gates'}
    if need - seen:
        bad.append('never staged: %s' % sorted(map(str, need - seen)))
    if len([k for k in seen if isinstance(k, tuple) and k[0] == 'wgate']) < 3:
        bad.append('fewer than three cases with per-gate weights')
    if not (TOP.n_gates == N_MAX and TOP.has_ice() and TOP.n_rays == 1) and cases is CASES:
        bad.append('no case with ice at the most gates')
    return bad
