"""Hydrometeor contributions: per gate and per hydrometeor species the reflectivities, ZDR, KDP, the specific attenuations,
RHOHV and DELTA_HV that the species ALONE would give, which species is present, which dominates ZH and by what share.

Replaces in the reference: nothing -- cosmo_pol folds the per-species sums with np.nansum(sz_integ, axis=1)
(doppler_scatter.py:400) and hands back the totals; its users re-run the sweep once per species with the others zeroed in the
model, which for the non-additive fields is also not the same thing.  The per-species sums are on the device already:
`sz_integ[gate][species][12]`, float32, formed by k_final / k_subbeam_sum.  The fields are made on the device behind the
sweep's kernels (k_species, cpol_species.inl), before the copy to the host; the pure host-side pieces live here so that they
are testable without a GPU: the specification and its refusals, and the NumPy statement of the rule that DEFINES what the kernel
computes (`fields_of`).  The operator's entry points are in radar_operator.py.

The rule.  Inputs: sz [n_rows, n_gates, n_hydro, 12] float32, the device's sz_integ -- a row of NaNs means that the species has
no item at the gate; zh_final [n_rows, n_gates] float32, the call's own ZH as delivered, after the range scans and the
sensitivity cut; three float32 constants formed as the launch sequence forms them: c_zh = float32(c_zh of the call),
c_kdp = float32(1e-3 * (180 / pi) * wavelength), c_2w = float32(2 * wavelength) (`constants_of`).
Per gate and species j, t[c] = sz[..., j, c]; every operation is ONE float32 operation, rounded on its own, unless stated:
    t[c] == 0 (either sign) becomes NaN                  (quirk Q5, applied to the species as the totals apply it)
    two_pi = float32(2 pi);  b = t0 - t1 - t2 + t3;  cc = t0 + t1 + t2 + t3   (left to right)
    ZH_j = c_zh * (two_pi * b);  ZV_j = c_zh * (two_pi * cc)
    ZDR_j = (two_pi * b) / (two_pi * cc)                 the INTRINSIC ratio: the total's ZDR is attenuated along the ray, a
                                                         species' ZDR is not (there is no per-species path)
    KDP_j = c_kdp * (t10 - t8)
    ATT_H_j = float32(4.343e-3) * (c_2w * t11);  ATT_V_j = float32(4.343e-3) * (c_2w * t9)
    RHOHV_j = sqrt(((t4 + t7) * (t4 + t7) + (t6 - t5) * (t6 - t5)) / (b * cc))
    DELTA_HV_j = float32(atan2(float64(t5 - t6), float64(-t4 - t7)))          (the differences in float32, atan2 in float64)
Censoring: where zh_final is NaN, ZH_j, ZV_j, ZDR_j, KDP_j and RHOHV_j become NaN for every j; ATT_H_j, ATT_V_j and DELTA_HV_j
keep their values -- exactly the set the sensitivity cut touches and leaves in the totals.
    present   uint8: bit j is set iff ZH_j == ZH_j after censoring
    dominant  uint8: starts at 255 with no best value; for j ascending, j is taken when bit j of `present` is set and either
              nothing has been taken yet or ZH_j > best (a strict float32 comparison: a tie keeps the lower slot)
    share     float32: S = the float32 sum of the ZH_j with bit j set, j ascending, starting from +0.0;
              share = ZH_dominant / S; NaN where dominant == 255
Nothing is special-cased: a negative b gives a negative ZH_j that counts as present, may be taken when it comes first, and enters
S with its sign; infinities give what IEEE gives."""
import numpy as np

# the per-species arrays of cpol_species, in the order of the struct
FIELDS = ('ZH', 'ZV', 'ZDR', 'KDP', 'RHOHV', 'DELTA_HV', 'ATT_H', 'ATT_V')
CUT_FIELDS = ('ZH', 'ZV', 'ZDR', 'KDP', 'RHOHV')      # what the sensitivity cut censors
PER_GATE = (('dominant', np.uint8), ('present', np.uint8), ('share', np.float32))
MAX_HYDRO = 8
N_SZ = 12
NONE = 255


class Species(object):
    """Which per-species fields: `fields` out of FIELDS; `dominant`: also 'dominant', 'present' and 'share' per gate; `raw`: also
    the rows themselves ('sz').  ValueError for an unknown field name and for nothing asked for at all."""

    def __init__(self, fields=('ZH', 'ZDR', 'KDP'), dominant=True, raw=False):
        if isinstance(fields, str):
            fields = (fields,)
        fields = tuple(fields)
        for k in fields:
            if k not in FIELDS:
                raise ValueError('Species: unknown field %r (known: %s)' % (k, ', '.join(FIELDS)))
        if not fields and not dominant and not raw:
            raise ValueError('Species: nothing asked for (no field, dominant=False, raw=False)')
        self.fields = tuple(k for k in FIELDS if k in fields)         # (the order of the struct)
        self.dominant, self.raw = bool(dominant), bool(raw)

    @property
    def key(self):
        return (self.fields, self.dominant, self.raw)

    def __repr__(self):
        return 'Species(fields=%r, dominant=%r, raw=%r)' % self.key


def constants_of(wavelength, k_squared):
    """(c_zh, c_kdp, c_2w) float32, as the launch sequence forms them from the call's float64 wavelength (the constants'
    WAVELENGTH) and the radar's K_squared."""
    wavelength, k_squared = float(wavelength), float(k_squared)
    c_zh = float(wavelength ** 4 / (np.pi ** 5 * k_squared))
    return (np.float32(c_zh), np.float32(1e-3 * (180.0 / 3.14159265358979323846) * wavelength), np.float32(2 * wavelength))


def names(hydrometeor_slots):
    """The species of a call in slot order, as a tuple of names (the leading axis of every per-species array)."""
    out = tuple(str(h) for h in hydrometeor_slots)
    if not 1 <= len(out) <= MAX_HYDRO:
        raise ValueError('species: 1 ... %d hydrometeor slots, got %d' % (MAX_HYDRO, len(out)))
    return out


def dominant_of(zh_species):
    """zh_species float32 [n_hydro, ...], censored -> {'present': uint8 [...], 'dominant': uint8 [...], 'share': float32 [...]}:
    the last three statements of the rule."""
    zh = np.asarray(zh_species)
    if zh.dtype != np.float32 or zh.ndim < 1 or not 1 <= zh.shape[0] <= MAX_HYDRO:
        raise ValueError('dominant_of: zh_species is float32 [n_hydro, ...] with 1 ... %d species' % MAX_HYDRO)
    lead = zh.shape[1:]
    present = np.zeros(lead, dtype=np.uint8)
    dominant = np.full(lead, NONE, dtype=np.uint8)
    best = np.zeros(lead, dtype=np.float32)
    total = np.zeros(lead, dtype=np.float32)
    with np.errstate(all='ignore'):
        for j in range(zh.shape[0]):
            here = zh[j] == zh[j]
            present = np.where(here, present | np.uint8(1 << j), present).astype(np.uint8)
            take = here & ((dominant == NONE) | (zh[j] > best))
            best = np.where(take, zh[j], best)
            dominant = np.where(take, np.uint8(j), dominant).astype(np.uint8)
            total = np.where(here, total + zh[j], total)
        share = np.where(dominant == NONE, np.float32(np.nan), best / total).astype(np.float32)
    return {'present': present, 'dominant': dominant, 'share': share}


def fields_of(sz, zh_final, c_zh, c_kdp, c_2w):
    """The rule in NumPy -- the slow way, and the definition of what k_species computes.  sz float32 [n_rows, n_gates, n_hydro,
    12], zh_final float32 [n_rows, n_gates], the three float32 constants -> {field: float32 [n_hydro, n_rows, n_gates] for every
    field of FIELDS, 'present', 'dominant': uint8 [n_rows, n_gates], 'share': float32 [n_rows, n_gates]}."""
    sz = np.asarray(sz)
    zh_final = np.asarray(zh_final)
    if sz.dtype != np.float32 or sz.ndim != 4 or sz.shape[3] != N_SZ or not 1 <= sz.shape[2] <= MAX_HYDRO:
        raise ValueError('fields_of: sz is float32 [n_rows, n_gates, n_hydro (1 ... %d), %d]' % (MAX_HYDRO, N_SZ))
    if zh_final.dtype != np.float32 or zh_final.shape != sz.shape[:2]:
        raise ValueError('fields_of: zh_final is float32 [n_rows, n_gates]')
    f32 = np.float32
    c_zh, c_kdp, c_2w = f32(c_zh), f32(c_kdp), f32(c_2w)
    with np.errstate(all='ignore'):
        t = np.where(sz == 0, f32(np.nan), sz)
        t = [np.ascontiguousarray(np.moveaxis(t[..., c], 2, 0)) for c in range(N_SZ)]     # each [n_hydro, n_rows, n_gates]
        two_pi = f32(2 * 3.14159265358979323846)
        b = t[0] - t[1] - t[2] + t[3]
        cc = t[0] + t[1] + t[2] + t[3]
        xs_h = two_pi * b
        xs_v = two_pi * cc
        out = {'ZH': c_zh * xs_h, 'ZV': c_zh * xs_v, 'ZDR': xs_h / xs_v, 'KDP': c_kdp * (t[10] - t[8]),
               'ATT_H': f32(4.343e-3) * (c_2w * t[11]), 'ATT_V': f32(4.343e-3) * (c_2w * t[9])}
        t47 = t[4] + t[7]
        t65 = t[6] - t[5]
        out['RHOHV'] = np.sqrt((t47 * t47 + t65 * t65) / (b * cc))
        out['DELTA_HV'] = np.arctan2((t[5] - t[6]).astype(np.float64), (-t[4] - t[7]).astype(np.float64)).astype(f32)
        cut = zh_final != zh_final
        for k in CUT_FIELDS:
            out[k] = np.where(cut[None], f32(np.nan), out[k])
    for k in FIELDS:
        assert out[k].dtype == np.float32, k
        out[k] = np.ascontiguousarray(out[k])
    out.update(dominant_of(out['ZH']))
    return out


class Contributions(object):
    """The hydrometeor contributions of ONE sweep call, as RadarOperator._run_rays takes a product ("How a product
    plugs into a sweep call").  `slots`: the staged hydrometeors in slot order.  The per-gate arrays of the sweep travel as in
    the plain call (`keep_gates`; ZH is made on the device either way: the censoring reads it)."""
    name = 'species'
    spectrum, model_var = True, None
    over_members = False
    refuses = {'members': 'hydrometeor contributions are taken by the plain and the time-blended sweeps: no ensemble call',
               'subbeams': 'hydrometeor contributions do not share a call with the sub-beam export',
               'groups': 'a species call needs one group (split the rays)'}

    def __init__(self, spec, slots, keep_gates=True, distributed=False):
        # what a species call refuses before it builds anything.  (Spaceborne geometry is refused by the ray calls themselves:
        # they take ground radars.)
        if not isinstance(spec, Species):
            raise ValueError('spec: a cosmo_pol_amd.species.Species, got %r' % (spec,))
        if distributed:
            raise NotImplementedError('hydrometeor contributions with a process group: sharding rays over ranks is not built')
        self.spec, self.gates = spec, bool(keep_gates)
        self.names = names(slots)

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        if n_members is not None:
            raise NotImplementedError(self.refuses['members'])
        self.sp = native.Context.species_struct(len(self.names))
        self.shape = (len(az), n_gates)
        return {'species': self.sp}, []

    def arrays(self):
        # in the sweep's own block: they ride the one copy
        out = [(k, np.float32, (len(self.names),) + self.shape) for k in self.spec.fields]
        if self.spec.dominant:
            out += [(k, dt, self.shape) for k, dt in PER_GATE]
        if self.spec.raw:
            out.append(('sz', np.float32, self.shape + (len(self.names), N_SZ)))
        return out

    def paths(self):
        return tuple(k for k, _, _ in self.arrays())

    def bind(self, path, address):
        if path not in FIELDS and path not in ('dominant', 'present', 'share', 'sz'):
            raise ValueError('species: no array %r' % (path,))
        setattr(self.sp, path, address)

    def bind_device(self, entry):         # {array name: device pointer}, the arrays of the spec and no other
        asked = self.paths()
        for k, ptr in entry.items():
            if k not in asked:
                raise ValueError("device_outputs['species']: unknown entry %r (the spec asks for %s)" % (k, ', '.join(asked)))
            self.bind(k, ptr)

    def finish(self, w, coords):
        out = {'names': self.names}
        out.update(w)
        return out

    def join(self, parts, cat):
        """Several results of one spec (the groups of a time-blended call are refused; kept for the interface): the rays joined."""
        out = {'names': self.names}
        for k in self.paths():
            out[k] = cat([q[k] for q in parts], axis=1 if k in FIELDS else 0)
        return out
