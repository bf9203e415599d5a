"""Hand-built columns for the counting sort and its work units (k_classify's rank tables, k_bucket_scan, k_bucket_scatter and the
unit walk of k_psd / k_psd_uniform / k_psd_melting[_tab] / k_psd_ice2, cosmo_pol_amd/csrc/cpol_psd.inl), and a host model of what
the sort must produce.

A sweep takes these stages whenever a slot has no integral table.  On interpolated radials temperature and elevation vary slowly
along a ray, so the rank tables never fill, buckets have the sizes chance gives them and no persistent grid ever strides.  Here
every such shape is BUILT: a scenario is a flat sequence of sub-beam gates ("slots", in the order of the device's arrays:
ray, sub-beam, gate) with chosen items; an item is (species, elevation bin, second-axis bin, palette entry).

  * T and the elevation of a slot sit at the CENTRE of the item's table bin (axis value + step / 2), the wet fraction of a melting
    item at the centre of its bin (float64; the last bin, which takes everything from 0.999 on, at the centre of [0.999, 1]: a
    wet fraction beyond 1 is no input of the melting scheme): the bin -- and with it the bucket key -- of an item is beyond doubt;
  * mass and number densities are drawn log-uniformly inside the range the golden radials span (Q_RANGE below, read off
    beam.interpolate_radial of the cases c2_rsg, c3_melt_ice, c3_dop2, c4_subbeams, c5_2mom and c5_2mom_dop2_sub), by a generator
    seeded with (scenario, species, key, palette entry): items of one bucket with the same palette entry have IDENTICAL inputs
    and must give identical bits wherever the sort puts them -- the first or the second slot of a lane, another unit of the
    bucket, a unit of 1 beside units of 128, another classify workgroup, a slot ticket in one workgroup and a direct claim in
    another -- while the entries of a palette differ by up to decades, so an item that received another item's result shows
    against the reference.  (The order inside a bucket comes from atomics and differs from run to run: planting by position
    is not possible, planting by palette is);
  * a slot holds at most one species of R / S / G / H / I (they share T) and, in the melting configurations, any of mS / mG beside
    it (their second axis is the wet fraction); all items of a slot share the elevation bin;
  * the melting fields are GIVEN (QmS_v, QmG_v, fwet_*, has_melting = 1 everywhere): presence is exactly what the builder says.

The configurations are existing radial cases (gen_golden.RADIAL_CASES) with the synthetic tables of _cases.synthetic_lut (8
elevations; 27 temperatures for rain, 39 for S / G / H / I, 100 wet fractions for mS / mG): c2_rsg has 840 keys (k_bucket_scan: one key
per thread), c3_melt_ice and c3_dop2 2752 (three per thread), c5_2mom 1464 (two per thread; the only one whose species differ in
their unit size: R and H 128 items, S, G, I 64).

host_model(scn) restates the sort from the columns alone: keys by the oracle's bin_index plus the per-species base (as
tests/test_gpu_parity.py does), the histogram, log2(items per unit) by the rule of cosmo_pol_hip.hip (where sa.unit_shift is
set) on the descriptor hydrometeors.build_hydro returns, and the unit count sum_k ceil(c_k / 2^shift).

ice_mixed_unit: lambda = (M2 / QM)^(1 / (b - 2)) of the 1-moment ice crystals leaves the normalisation tables' range
2^ICE_LOG2_LO .. 2^ICE_LOG2_HI upwards for small mass densities (QI = 1e-20 at 239 K: log2(lambda) = 15.35, N0 finite), so the
scenario exists: its odd item is the one mass density outside Q_RANGE, searched by ice_q_outside()."""
import copy
import functools
import zlib

import numpy as np

import _cases
from cosmo_pol_oracle import config as ocfg

GG = _cases.gen_golden

# [lowest, highest] positive value of the golden radials (module docstring), rounded outwards to two digits
Q_RANGE = {'QR_v': (3.0e-9, 2.0e-3), 'QS_v': (1.6e-8, 9.1e-4), 'QG_v': (2.4e-8, 6.5e-4), 'QI_v': (1.0e-9, 1.9e-5),
           'QH_v': (3.3e-7, 6.4e-6), 'QmS_v': (4.1e-4, 2.2e-3), 'QmG_v': (1.0e-7, 6.5e-4),
           'QNR_v': (2.7e-2, 1.1e5), 'QNS_v': (2.8, 1.3e3), 'QNG_v': (2.3e-2, 9.2e2), 'QNH_v': (0.12, 3.2),
           'QNI_v': (3.4e3, 5.0e5)}
MELTING = ('mS', 'mG')
N_SUB, N_GATES = 3, 100                  # no multiple of 256: the classify workgroups straddle sub-beams and rays
CLASSIFY_THREADS = 256                   # CPOL_CLASSIFY_THREADS: sub-beam gates per k_classify workgroup
RANK_SLOTS = 128                         # CPOL_RANK_SLOTS
WINDOW = 192                             # the overflow scenarios hold for any window of this length, whatever the workgroup width
EDGE_COUNTS = (1, 63, 64, 65, 127, 128, 129, 257)
PALETTE = 3
T_DEFAULT = np.float32(269.0)            # slots without a species that reads T (inside every table's axis)


def q_name(h):
    return 'Q' + h + '_v'


@functools.lru_cache(maxsize=None)
def setup(case):
    """-> (config override, oracle config, species, {h: table}, variable names, two-moment?)"""
    over, _, _, _, two = GG.radial_case_inputs(case)       # (the override with the cases' radar site and defaults; its cube is unused)
    over = copy.deepcopy(over)
    conf = ocfg.make_config(copy.deepcopy(over))
    hl = tuple(ocfg.hydrometeor_list(conf))
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in hl}
    names = tuple(_cases.ORDER_2MOM if two else _cases.ORDER)
    return over, conf, hl, luts, names, two


@functools.lru_cache(maxsize=None)
def key_layout(case):
    """-> (n_e [nh], n_t [nh], key_base [nh + 1])"""
    _, _, hl, luts, _, _ = setup(case)
    n_e = [luts[h].value_table.shape[0] for h in hl]
    n_t = [luts[h].value_table.shape[1] for h in hl]
    base = np.concatenate([[0], np.cumsum([a * b for a, b in zip(n_e, n_t)])]).astype(int)
    return tuple(n_e), tuple(n_t), tuple(int(b) for b in base)


@functools.lru_cache(maxsize=None)
def unit_shifts(case):
    """log2(items per work unit) per species: cosmo_pol_hip.hip, `sa.unit_shift[j] = ...` -- 7 for the gamma species on a uniform
    diameter grid, the melting species with their wet-fraction tables and the 1-moment ice crystals on a uniform grid with their
    normalisation tables, 6 otherwise."""
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import hydrometeors as H
    _, conf, hl, luts, names, _ = setup(case)
    vi = {v: i for i, v in enumerate(names)}
    out = []
    for h in hl:
        d = H.build_hydro(h, conf['microphysics']['scheme'], luts[h], vi)[0]
        two_per_lane = (d.psd_family == N.PSD_GAMMA and d.uniform_grid) or \
                       (d.psd_family == N.PSD_MELTING and d.tab_degree == N.MELT_DEGREE) or \
                       (d.psd_family == N.PSD_ICE_FIELD and d.uniform_grid and d.tab_degree == N.ICE_DEGREE)
        out.append(7 if two_per_lane else 6)
    return tuple(out)


class Scenario(object):
    """name, case; n_rays x N_SUB x N_GATES columns (`cols`, read-only), the designed key per (species, slot) (`design`, -1:
    no item), the palette entry per (species, slot) (`palette`) and whatever the builder notes in `notes`."""

    def __init__(self, name, case):
        self.name, self.case = name, case
        self.over, self.conf, self.species, self.luts, self.names, self.two = setup(case)
        self._items = {}                      # (slot, j) -> (eb, tb, pal, q or None)
        self._eb = {}                         # slot -> eb
        self._gamma = {}                      # slot -> j of the species that fixes T
        self.notes = {}
        self.cols = None

    # ---- building ----
    def put(self, slot, h, eb, tb, pal=0, q=None):
        j = self.species.index(h)
        n_e, n_t, _ = key_layout(self.case)
        assert 0 <= eb < n_e[j] and 0 <= tb < n_t[j], (h, eb, tb)
        assert (slot, j) not in self._items, (slot, h)
        assert self._eb.setdefault(slot, eb) == eb, 'the items of a slot share the elevation bin'
        if h not in MELTING:
            assert self._gamma.setdefault(slot, j) == j, 'one species that reads T per slot'
        self._items[(slot, j)] = (eb, tb, pal, q)

    def finish(self, n_slots=None):
        nh = len(self.species)
        top = max([s for s, _ in self._items] + [0]) + 1
        n_slots = max(top, n_slots or 0, 1)
        per_ray = N_SUB * N_GATES
        self.n_rays, self.n_sub, self.n_gates = -(-n_slots // per_ray), N_SUB, N_GATES
        n = self.n_sbg = self.n_rays * per_ray
        n_e, n_t, base = key_layout(self.case)
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        flat = {k: np.zeros(n, dtype=np.float32) for k in self.names}
        flat['U'] = rng.uniform(-20.0, 20.0, n).astype(np.float32)
        flat['V'] = rng.uniform(-15.0, 15.0, n).astype(np.float32)
        flat['W'] = rng.uniform(-2.0, 2.0, n).astype(np.float32)
        flat['RHO'] = rng.uniform(0.6, 1.2, n).astype(np.float32)
        flat['T'][:] = T_DEFAULT
        elev = np.ones(n, dtype=np.float32)
        melt = bool(self.conf['microphysics']['with_melting'])
        if melt:
            for h in MELTING:
                flat[q_name(h)] = np.zeros(n, dtype=np.float32)
                flat['fwet_' + h] = np.full(n, 0.5, dtype=np.float64)
        self.design = np.full((nh, n), -1, dtype=np.int32)
        self.palette = np.full((nh, n), -1, dtype=np.int8)
        for (slot, j), (eb, tb, pal, q) in sorted(self._items.items()):
            h = self.species[j]
            L = self.luts[h]
            key = base[j] + eb * n_t[j] + tb
            self.design[j, slot], self.palette[j, slot] = key, pal
            ax_e = L.axes_names['e']
            elev[slot] = np.float32(L.axes_limits[ax_e][0]) + np.float32(L.axes_step[ax_e]) * np.float32(eb + 0.5)
            draw = np.random.default_rng(zlib.crc32(('%s/%s/%d/%d' % (self.name, h, key, pal)).encode()))
            lo, hi = Q_RANGE[q_name(h)]
            qv = np.float32(np.exp(draw.uniform(np.log(lo), np.log(hi))))
            flat[q_name(h)][slot] = qv if q is None else np.float32(q)
            if self.two:
                lo, hi = Q_RANGE['QN' + h + '_v']
                flat['QN' + h + '_v'][slot] = np.float32(np.exp(draw.uniform(np.log(lo), np.log(hi))))
            if h in MELTING:
                ax = L.axes_names['wc']
                lo_edge = np.float64(L.axes_limits[ax][0]) + np.float64(L.axes_step[ax]) * tb
                # (the last bin takes everything from 0.999 on, and a wet fraction ends at 1: its centre is that of [0.999, 1])
                flat['fwet_' + h][slot] = min(lo_edge + np.float64(L.axes_step[ax]) * 0.5, (lo_edge + 1.0) / 2)
            else:
                ax = L.axes_names['t']
                flat['T'][slot] = np.float32(L.axes_limits[ax][0]) + np.float32(L.axes_step[ax]) * np.float32(tb + 0.5)
        shape = (self.n_rays, self.n_sub, self.n_gates)
        cols = {k: v.reshape(shape) for k, v in flat.items()}
        cols['elev'] = elev.reshape(shape)
        if melt:
            cols['has_melting'] = np.ones((self.n_rays, self.n_sub), dtype=np.int8)
        s = np.arange(self.n_sub)
        cols['quad_weights'] = (1.0 + 0.4 * ((7 * s) % 131) / 131.0) / self.n_sub          # distinct, of one magnitude
        cols['quad_pts'] = np.ascontiguousarray(np.stack(
            [np.broadcast_to(10.0 * np.arange(self.n_rays)[:, None] + 0.5 * s[None, :], (self.n_rays, self.n_sub)),
             np.broadcast_to(1.0 + 0.3 * s[None, :], (self.n_rays, self.n_sub))], axis=-1))
        for a in cols.values():
            a.setflags(write=False)
        self.cols = cols
        del self._items, self._eb, self._gamma
        return self

    # ---- reading ----
    def flat(self, name):
        return self.cols[name].reshape(-1)

    def subbeams(self, ray, radial_res=None):
        """The oracle's sub-radials of one ray (fresh arrays: the oracle folds elevations in place)."""
        from cosmo_pol_oracle.beam import SubBeam
        ng, cols = self.n_gates, self.cols
        res = self.conf['radar']['radial_resolution'] if radial_res is None else radial_res
        melt = 'has_melting' in cols
        subs = []
        for s in range(self.n_sub):
            values = {k: np.array(cols[k][ray, s], dtype=np.float32) for k in self.names}
            if melt:
                for h in MELTING:
                    values[q_name(h)] = np.array(cols[q_name(h)][ray, s], dtype=np.float64)
                    values['fwet_' + h] = np.array(cols['fwet_' + h][ray, s], dtype=np.float64)
            sb = SubBeam(values, np.zeros(ng), np.zeros(ng), np.zeros(ng), res * (0.5 + np.arange(ng)), np.zeros(ng),
                         elev=np.array(cols['elev'][ray, s], dtype=np.float32),
                         quad_pt=[float(x) for x in cols['quad_pts'][ray, s]], quad_weight=np.float64(cols['quad_weights'][s]))
            if melt:
                sb.has_melting = bool(cols['has_melting'][ray, s])
            subs.append(sb)
        return subs

    def __repr__(self):
        return '%s[%s]' % (self.name, self.case)


# ---------------------------------------------------------------- the host model
def host_model(scn):
    """From the columns alone -> dict(keys [nh, n_sbg] (-1: no item), hist [n_keys], n_valid, shifts [nh], n_units, key_base)."""
    nh = len(scn.species)
    _, n_t, base = key_layout(scn.case)
    keys = np.full((nh, scn.n_sbg), -1, dtype=np.int32)
    elev = scn.flat('elev')
    for j, h in enumerate(scn.species):
        L = _cases.as_oracle_lut(scn.luts[h])
        q = scn.flat(q_name(h))
        valid = q > 0
        if h in MELTING:
            valid = valid & np.repeat(scn.cols['has_melting'].reshape(-1) != 0, scn.n_gates)
        if valid.any():
            eb = L.bin_index('e', elev[valid])
            tb = (L.bin_index('wc', scn.flat('fwet_' + h)[valid]) if h in MELTING else L.bin_index('t', scn.flat('T')[valid]))
            keys[j, valid] = base[j] + eb * n_t[j] + tb
    hist = np.bincount(keys[keys >= 0], minlength=base[-1]).astype(np.int64)
    shifts = unit_shifts(scn.case)
    n_units = 0
    for j in range(nh):
        c = hist[base[j]:base[j + 1]]
        n_units += int(np.sum(-(-c // (1 << shifts[j]))))
    return dict(keys=keys, hist=hist, n_valid=int((keys >= 0).sum()), shifts=shifts, n_units=n_units, key_base=base)


def distinct_per_window(keys_j, start, stop, width=WINDOW):
    """Distinct keys >= 0 of one species in every window [p, p + width) inside [start, stop) -> array."""
    out = []
    for p in range(start, stop - width + 1):
        w = keys_j[p:p + width]
        out.append(len(np.unique(w[w >= 0])))
    return np.array(out)


def item_reference(scn, chunk=256):
    """float64 [nh, n_sbg, 12]: every item's PSD-integrated scattering entries recomputed from the oracle's own parts
    (create_hydrometeor, set_psd, get_N, lookup_line, the einsum of scatter.radar_observables) BEFORE the sub-beam weight and the
    float32 store; NaN where there is no item.  Items with identical inputs are computed once."""
    from cosmo_pol_oracle.psd import create_hydrometeor, vlinspace
    scheme = scn.conf['microphysics']['scheme']
    keys = host_model(scn)['keys']
    out = np.full((len(scn.species), scn.n_sbg, 12), np.nan)
    elev, T = scn.flat('elev'), scn.flat('T')
    for j, h in enumerate(scn.species):
        idx = np.where(keys[j] >= 0)[0]
        if not len(idx):
            continue
        L = _cases.as_oracle_lut(scn.luts[h])
        hyd = create_hydrometeor(h, scheme)
        hyd.nbins_D = L.value_table.shape[-2]
        d_ax = L.axes[2]
        hyd.d_min = d_ax[:, 0] if h in MELTING else d_ax[0]
        hyd.d_max = d_ax[:, -1] if h in MELTING else d_ax[-1]
        q = scn.flat(q_name(h))
        ident = [elev[idx].astype(np.float64), T[idx].astype(np.float64), q[idx].astype(np.float64)]
        if scn.two:
            ident.append(scn.flat('QN' + h + '_v')[idx].astype(np.float64))
        if h in MELTING:
            ident.append(scn.flat('fwet_' + h)[idx])
        _, first, inverse = np.unique(np.stack(ident, axis=1), axis=0, return_index=True, return_inverse=True)
        rep = idx[first]
        vals = np.empty((len(rep), 12))
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            for a in range(0, len(rep), chunk):
                g = rep[a:a + chunk]
                e, t = elev[g].copy(), T[g].copy()
                if scheme == '1mom':
                    if h == 'mG':
                        fw = scn.flat('fwet_' + h)[g]
                        hyd.set_psd(q[g].astype(np.float64), fw)
                    elif h == 'mS':
                        fw = scn.flat('fwet_' + h)[g]
                        hyd.set_psd(t, q[g].astype(np.float64), fw)
                    elif h in ('S', 'I'):
                        hyd.set_psd(t, q[g])
                    else:
                        hyd.set_psd(q[g])
                else:
                    hyd.set_psd(scn.flat('QN' + h + '_v')[g], q[g])
                if h in MELTING:
                    list_D = vlinspace(hyd.d_min, hyd.d_max, hyd.nbins_D)
                    dD = list_D[:, 1] - list_D[:, 0]
                    sz = L.lookup_line(e=e, wc=fw)
                    vals[a:a + chunk] = np.einsum('ijk,ij->ik', sz, hyd.get_N(list_D)) * dD[:, None]
                else:
                    list_D = L.axes[L.axes_names['d']]
                    dD = list_D[1] - list_D[0]
                    N = hyd.get_N(list_D)
                    if N.ndim == 1:
                        N = N.reshape(len(N), 1)
                    sz = L.lookup_line(e=e, t=t)
                    vals[a:a + chunk] = np.einsum('ijk,ij->ik', sz, N) * dD
        out[j, idx] = vals[np.reshape(inverse, -1)]
    return out


def solo(scn, slot, j, at=None):
    """The item (species j of `slot`) alone in a call of one ray: its inputs copied to the slot `at` (default: the last sub-beam
    gate), every other mass density 0 -> columns, and the flat index of the item."""
    per_ray = scn.n_sub * scn.n_gates
    at = per_ray - 1 if at is None else at
    h = scn.species[j]
    shape = (1, scn.n_sub, scn.n_gates)
    cols = {}
    for k, v in scn.cols.items():
        if k in ('quad_weights',):
            cols[k] = v
        elif k in ('quad_pts', 'has_melting'):
            cols[k] = np.ascontiguousarray(v[:1])
        else:
            f = v.reshape(-1)[:per_ray].copy()
            if k.startswith('Q'):
                f[:] = 0
            mine = k in ('T', 'elev', q_name(h), 'QN' + h + '_v', 'fwet_' + h)
            if mine:
                f[at] = v.reshape(-1)[slot]
            cols[k] = f.reshape(shape)
    return cols, at


# ---------------------------------------------------------------- scenarios
def _split_key(case, h, k):
    """k-th key of species h -> (eb, tb)"""
    _, _, hl, _, _, _ = setup(case)
    n_t = key_layout(case)[1][hl.index(h)]
    return k // n_t, k % n_t


def _overflow(name, case, named):
    """Stretch A = [0, 1024): three slots of four walk through the keys of the named species one by one (144 distinct keys of each
    in any 192 slots, 192 in a workgroup of 256: above the 128 slots of its rank table), the fourth repeats the slot three
    before it -- slot tickets and direct claims for one species side by side in every workgroup.  Stretch B = [1024, 1024 + 4 x
    keys): four slots per key, at most 65 distinct keys in any 256 slots -- every key is ranked through a slot there, so each of
    the (at least 64 per workgroup of A) directly claimed keys is claimed through a slot by another workgroup."""
    scn = Scenario(name, case)
    nk = min(key_layout(case)[0][scn.species.index(h)] * key_layout(case)[1][scn.species.index(h)] for h in named)
    len_a = 1024

    def place(slot, c, pal):
        eb = None
        for h in named:
            if h in MELTING:
                # (eb, c mod 100) is distinct over c < 216: c and c + 100 differ in c // 27
                e, t = (c // 27) % 8, c % 100
            else:
                e, t = _split_key(case, h, c % nk)
            eb = e if eb is None else eb
            scn.put(slot, h, eb, t, pal)
    nk = min(nk, 216)                       # (the walk of a melting species is tied to the 8 x 27 pattern of (eb, c mod 100))
    for p in range(len_a):
        if p % 4 == 3:
            place(p, (3 * ((p - 3) // 4)) % nk, 1)           # the repeat of slot p - 3, another palette entry
        else:
            place(p, (3 * (p // 4) + p % 4) % nk, 0)
    for p in range(4 * nk):
        place(len_a + p, p // 4, p % PALETTE)
    scn.notes.update(named=named, stretch_a=(0, len_a), stretch_b=(len_a, len_a + 4 * nk), n_walk=nk)
    return scn.finish()


def _spread(scn, items, seed):
    """One item per slot, in an order shuffled once: the items of a bucket end up in many workgroups and rays."""
    order = np.random.default_rng(seed).permutation(len(items))
    for slot, i in enumerate(order):
        h, eb, tb, pal = items[i]
        scn.put(slot, h, eb, tb, pal)
    return scn.finish()


def _unit_edges(name, case):
    scn = Scenario(name, case)
    n_e, n_t, _ = key_layout(case)
    items, buckets = [], {}
    for j, h in enumerate(scn.species):
        nk = n_e[j] * n_t[j]
        for i, c in enumerate(EDGE_COUNTS):
            eb, tb = _split_key(case, h, (i * nk) // len(EDGE_COUNTS) + 3 + j)
            buckets[(h, eb, tb)] = c
            items += [(h, eb, tb, m % PALETTE) for m in range(c)]
    scn.notes['buckets'] = buckets
    return _spread(scn, items, 11)


def _species_borders(name, case):
    scn = Scenario(name, case)
    n_e, n_t, _ = key_layout(case)
    items, buckets = [], {}
    for j, h in enumerate(scn.species):
        for (eb, tb), c in (((0, 0), 65), ((n_e[j] - 1, n_t[j] - 1), 129)):
            buckets[(h, eb, tb)] = c
            items += [(h, eb, tb, m % PALETTE) for m in range(c)]
    scn.notes['buckets'] = buckets
    return _spread(scn, items, 12)


def scan_border_keys(n_keys):
    """k_bucket_scan: thread t owns the keys [t per, (t + 1) per), per = ceil(n_keys / 1024): key 0, the last key, and the keys on
    either side of the borders of threads 1, 512, 1023 and of the last thread that owns a key (those that exist)."""
    per = -(-n_keys // 1024)
    last_t = (n_keys - 1) // per
    want = {0, n_keys - 1}
    for t in (1, 512, 1023, last_t):
        want |= {t * per - 1, t * per}
    return per, sorted(k for k in want if 0 <= k < n_keys)


def _scan_borders(name, case):
    scn = Scenario(name, case)
    n_e, n_t, base = key_layout(case)
    per, keys = scan_border_keys(base[-1])
    counts = (65, 129, 1, 64, 128, 63, 127, 2)
    items, buckets = [], {}
    for i, k in enumerate(keys):
        j = max(q for q in range(len(scn.species)) if base[q] <= k)
        eb, tb = divmod(k - base[j], n_t[j])
        c = counts[i % len(counts)]
        buckets[(scn.species[j], eb, tb)] = c
        items += [(scn.species[j], eb, tb, m % PALETTE) for m in range(c)]
    scn.notes.update(buckets=buckets, per=per, keys=keys)
    return _spread(scn, items, 13)


def _many_units(name, case):
    """Every key of the six species: per elevation bin 144 slots carry the 27 + 39 + 39 + 39 keys of R, S, G, I, the first 100 of
    them the 100 keys of mS and (in the opposite order) of mG.  One unit per key: more units than any persistent grid has
    workgroups (1024)."""
    scn = Scenario(name, case)
    n_e, n_t, _ = key_layout(case)
    assert scn.species == ('R', 'S', 'G', 'mS', 'mG', 'I')
    slot = 0
    for eb in range(8):
        local = 0
        for h in ('R', 'S', 'G', 'I'):
            for tb in range(n_t[scn.species.index(h)]):
                scn.put(slot, h, eb, tb, 0)
                if local < 100:
                    scn.put(slot, 'mS', eb, local, 0)
                    scn.put(slot, 'mG', eb, 99 - local, 0)
                slot += 1
                local += 1
    return scn.finish()


SPARSE_RANKED = (5, 300, 777, 1500, 1535)        # slots of the melting items: classify workgroups 0, 1, 3 and 5 of 8
SPARSE_SLOTS = 6 * N_SUB * N_GATES


def _sparse_blocks(name, case, previous=False):
    """Rain in every slot of 6 rays (runs of tabulated items under CPOL_ITAB_MELT=0), melting snow and graupel in five isolated
    slots: the classify workgroups 2, 4, 6 and 7 rank nothing there.  `previous`: the call to make BEFORE it on the same context --
    the same slots, the rain of every slot at 1e-22 .. 5e-22 kg m-3 (log2 of its PSD slope is above 14, the integral table of rain
    ends at 12.75: every rain item is ranked and pos[] of every gate holds a position), no melting items."""
    scn = Scenario(name, case)
    for slot in range(SPARSE_SLOTS):
        c = (slot * 7) % 216
        if previous:
            scn.put(slot, 'R', c // 27, c % 27, slot % PALETTE, q=1e-22 * (1 + slot % 5))
        else:
            scn.put(slot, 'R', c // 27, c % 27, slot % PALETTE)
            if slot in SPARSE_RANKED:
                scn.put(slot, 'mS', c // 27, (slot * 3) % 100, 0)
                scn.put(slot, 'mG', c // 27, (slot * 5) % 100, 0)
    scn.notes['ranked_slots'] = SPARSE_RANKED
    return scn.finish()


ICE_MIXED_KEY = (3, 19)                  # (elevation bin, temperature bin): T = 239 K
ICE_PLAIN_KEY = (5, 19)


def ice_log2_lambda(T, q):
    from cosmo_pol_oracle.psd import create_hydrometeor
    ice = create_hydrometeor('I', '1mom')
    with np.errstate(all='ignore'):
        ice.set_psd(np.atleast_1d(np.float32(T)), np.atleast_1d(np.float32(q)))
        return float(np.log2(ice.lambda_[0])), float(ice.N0[0])


def ice_q_outside(T):
    """The largest power of ten QI (float32, kg m-3) whose lambda at temperature T lies above 2^ICE_LOG2_HI with half an octave to
    spare and a finite, positive intercept; None if there is none."""
    from cosmo_pol_amd import hydrometeors as H
    for e in range(-10, -38, -1):
        l2, n0 = ice_log2_lambda(T, 10.0 ** e)
        if l2 > H.ICE_LOG2_HI + 0.5:
            return np.float32(10.0 ** e) if np.isfinite(n0) and n0 > 0 else None
    return None


def _ice_mixed_unit(name, case):
    """Two ice buckets of 64 items (one unit each): in the first, one item's lambda lies outside the normalisation tables -- the
    unit fails ice_unit_in_table, k_psd_ice2 leaves it to k_psd<ICE> and raises totals[2]; the second stays with k_psd_ice2."""
    scn = Scenario(name, case)
    L = scn.luts['I']
    ax = L.axes_names['t']
    T = float(L.axes_limits[ax][0]) + float(L.axes_step[ax]) * (ICE_MIXED_KEY[1] + 0.5)
    q_out = ice_q_outside(T)
    assert q_out is not None
    items = [('I',) + ICE_MIXED_KEY + (m % PALETTE,) for m in range(63)] + [('I',) + ICE_PLAIN_KEY + (m % PALETTE,) for m in range(64)]
    order = np.random.default_rng(14).permutation(len(items))
    for slot, i in enumerate(order):
        scn.put(slot, *items[i])
    odd = len(items) + 40
    scn.put(odd, 'I', ICE_MIXED_KEY[0], ICE_MIXED_KEY[1], PALETTE, q=q_out)
    scn.notes.update(odd_slot=odd, q_outside=float(q_out), T=T,
                     buckets={('I',) + ICE_MIXED_KEY: 64, ('I',) + ICE_PLAIN_KEY: 64})
    return scn.finish()


def _empty(name, case):
    return Scenario(name, case).finish(N_SUB * N_GATES)


def _one_item(name, case):
    scn = Scenario(name, case)
    scn.put(N_SUB * N_GATES - 1, 'S', 4, 20, 0)
    return scn.finish()


# name -> (builder, case, extra arguments).  Doppler scheme 2 (the DOP2 instantiations, vn): the c3_dop2 scenarios; scheme 1: the others.
BUILDERS = {
    'overflow_R': (_overflow, 'c2_rsg', (('R',),)),
    'overflow_mS': (_overflow, 'c3_dop2', (('mS',),)),
    'overflow_two_species': (_overflow, 'c3_melt_ice', (('R', 'mS'),)),
    'unit_edges_1mom': (_unit_edges, 'c3_dop2', ()),
    'unit_edges_2mom': (_unit_edges, 'c5_2mom', ()),
    'species_borders_1mom': (_species_borders, 'c3_melt_ice', ()),
    'species_borders_2mom': (_species_borders, 'c5_2mom', ()),
    'scan_borders_per1': (_scan_borders, 'c2_rsg', ()),
    'scan_borders_per3': (_scan_borders, 'c3_melt_ice', ()),
    'many_units': (_many_units, 'c3_melt_ice', ()),
    'sparse_blocks': (_sparse_blocks, 'c3_melt_ice', ()),
    'ice_mixed_unit': (_ice_mixed_unit, 'c3_melt_ice', ()),
    'empty': (_empty, 'c3_melt_ice', ()),
    'one_item': (_one_item, 'c3_melt_ice', ()),
}
SCENARIOS = tuple(BUILDERS)
MELTING_SCENARIOS = tuple(n for n, b in BUILDERS.items() if b[1] in ('c3_melt_ice', 'c3_dop2') and n not in ('empty',))
STALE_SEQUENCE = ('many_units', 'one_item', 'empty', 'unit_edges_1mom')      # on one operator, all as c3_melt_ice


@functools.lru_cache(maxsize=None)
def scenario(name, case=None):
    """The scenario `name` (computed once and shared, read-only); `case`: another configuration than the registered one."""
    if name == 'sparse_blocks_previous':
        return _sparse_blocks(name, case or 'c3_melt_ice', previous=True)
    fn, default, args = BUILDERS[name]
    return fn(name, case or default, *args)
