"""Superobservations: the per-gate fields of a call averaged over windows of a few rays by a few gates.

Replaces in the reference: nothing -- cosmo_pol hands back one value per range gate.  A data-assimilation system takes
radar data as superobservations: window averages with the number of gates that went into each.  The averaging runs on
the device behind the sweep's kernels (k_superob, cpol_superob.inl), before the copy to the host; the pure host-side
pieces live here so that they are testable without a GPU: the window specification and its refusals, the shape of the
result, the NumPy statement of the rule that DEFINES what the kernel computes (`average`), and the window means of the
gate coordinates.  The operator's entry points are in radar_operator.py.

The rule.  The per-gate fields form n_rows rows of n_gates gates (n_rows = n_rays, or n_members * n_rays for an ensemble
call).  Windows tile the rows in blocks of `rays_per_block` rows (0: all rays of the call): window row i of a block
holds its rays [i R, min((i + 1) R, rays_per_block)), window column j the gates [j G, min((j + 1) G, n_gates)).  A window
never crosses a block; the last windows of a block or a row may be partial; rays are taken in the order of the call (no
azimuth wrap-around).  Per field (ZH, ZV, KDP, DELTA_HV, PHIDP, RHOHV, ATT_H, ATT_V: float32; RVEL: float64):
    a gate counts when its value is not NaN; n = the counting gates of the window
    s_r = the float64 sum of the counting values of ray r in ascending gate order, from +0.0
    S   = the float64 sum of the s_r in ascending ray order, from +0.0
    the superobservation is S / n (float64), rounded once to float32 for the float32 fields
    NaN when n < need = max(1, int(ceil(min_valid_fraction * N))), N = the gates the window actually holds
ZDR is the ratio of the window's mean powers, not the mean of the ratios (an antenna averaging over the window measures
power): over the gates where ZH and ZV both count, S_H and S_V by the rule above, ZDR = float32(S_H / S_V), n = those
gates.  `count[field]` is n as uint16 (so R * G <= 65535).  mask, model variables and the Doppler spectrum are not
averaged.  RVEL after aliasing: the mean is the mean of the FOLDED velocities; nothing is unfolded."""
import math

import numpy as np

# the rows of cpol_superob.count, in this order
FIELDS = ('ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL')
COORDINATES = ('lats', 'lons', 'dist', 'heights')
MAX_WINDOW = 65535


class Superob(object):
    """A window specification: `rays` x `gates` per superobservation, NaN where fewer than `min_valid_fraction` of a
    window's gates count.  ValueError for what the library refuses with CPOL_ERR_ARG: a window < 1, rays * gates >
    65535, a fraction outside (0, 1] or NaN."""

    def __init__(self, rays, gates, min_valid_fraction=0.5):
        if int(rays) != rays or int(gates) != gates:
            raise ValueError('Superob: rays and gates must be integers, got %r x %r' % (rays, gates))
        rays, gates = int(rays), int(gates)
        if rays < 1 or gates < 1:
            raise ValueError('Superob: a window needs at least one ray and one gate, got %d x %d' % (rays, gates))
        if rays * gates > MAX_WINDOW:
            raise ValueError('Superob: rays * gates = %d > %d (the count of a window is uint16)' % (rays * gates, MAX_WINDOW))
        f = float(min_valid_fraction)
        if not (f > 0.0 and f <= 1.0):
            raise ValueError('Superob: min_valid_fraction %r outside (0, 1]' % (min_valid_fraction,))
        self.rays, self.gates, self.min_valid_fraction = rays, gates, f

    @property
    def key(self):
        return (self.rays, self.gates, self.min_valid_fraction)

    def __repr__(self):
        return 'Superob(%d, %d, min_valid_fraction=%r)' % self.key


def _block(n_rows, n_rays, rays_per_block):
    rpb = int(rays_per_block)
    if rpb < 0:
        raise ValueError('rays_per_block %d < 0' % rpb)
    rpb = rpb or int(n_rays)
    if rpb < 1 or n_rows % rpb:
        raise ValueError('rays_per_block %d does not divide the %d rows of the call' % (rpb, n_rows))
    return rpb


def shape(n_rays, n_gates, spec, rays_per_block=0):
    """(window rows, window columns) of a call of n_rays rows: (n_rays / rays_per_block) * ceil(rays_per_block / R) by
    ceil(n_gates / G), the blocks stacked in row order."""
    rpb = _block(int(n_rays), int(n_rays), rays_per_block)
    return (n_rays // rpb) * (-(-rpb // spec.rays)), -(-int(n_gates) // spec.gates)


def _sums(x, counts, spec, rpb):
    """x, counts: [n_rows, n_gates] float64 values and which of them count -> (S, n, N) per window, [n_blocks * wr, wc]."""
    n_rows, n_gates = x.shape
    R, G = spec.rays, spec.gates
    nb, wr, wc = n_rows // rpb, -(-rpb // R), -(-n_gates // G)
    # padded to whole windows with gates that do not count and do not exist
    v = np.zeros((nb, wr * R, wc * G), dtype=np.float64)
    c = np.zeros((nb, wr * R, wc * G), dtype=bool)
    e = np.zeros((nb, wr * R, wc * G), dtype=bool)
    v[:, :rpb, :n_gates] = np.where(counts, x, 0.0).reshape(nb, rpb, n_gates)       # (a gate that does not count adds +0.0:
    c[:, :rpb, :n_gates] = counts.reshape(nb, rpb, n_gates)                         # s + 0.0 has the bits of s, s never being -0.0)
    e[:, :rpb, :n_gates] = True
    v = v.reshape(nb, wr, R, wc, G)
    with np.errstate(invalid='ignore', over='ignore'):
        s = np.zeros((nb, wr, R, wc), dtype=np.float64)
        for g in range(G):                                  # ascending gate order, one addition per gate
            s = s + v[..., g]
        S = np.zeros((nb, wr, wc), dtype=np.float64)
        for r in range(R):                                  # ascending ray order, one addition per ray
            S = S + s[:, :, r, :]
    n = np.count_nonzero(c.reshape(nb, wr, R, wc, G), axis=(2, 4))
    N = np.count_nonzero(e.reshape(nb, wr, R, wc, G), axis=(2, 4))
    return S.reshape(nb * wr, wc), n.reshape(nb * wr, wc), N.reshape(nb * wr, wc)


def average(fields, spec, rays_per_block=0):
    """The rule at the top of this module in NumPy, statement by statement: `fields` {name: [n_rays, n_gates] or
    [n_members, n_rays, n_gates]} per-gate arrays (of FIELDS; others are ignored; ZDR is made from ZH and ZV when both are
    there, the per-gate ZDR is not read) -> {name: [(n_members,) window rows, window columns]} in the dtype of the per-gate
    field, and 'count': {name: uint16 array}.  The slow way to a superobservation, and the definition of what k_superob
    computes: the device result carries these bits."""
    out, count = {}, {}
    lead = None

    def rows(a):
        a = np.asarray(a)
        if a.ndim not in (2, 3):
            raise ValueError('average: per-gate fields are [n_rays, n_gates] or [n_members, n_rays, n_gates]')
        return a.reshape(-1, a.shape[-1]), a.shape

    def finish(S, n, N, dtype, ratio_of=None):
        need = np.maximum(1, np.ceil(spec.min_valid_fraction * N.astype(np.float64)).astype(np.int64))
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            q = (S / n.astype(np.float64) if ratio_of is None else S / ratio_of).astype(dtype)
        q[n < need] = np.nan
        return q, n.astype(np.uint16)

    def shaped(a, shp):
        return a if len(shp) == 2 else a.reshape((shp[0], -1, a.shape[-1]))

    for k in FIELDS:
        if k == 'ZDR':
            if 'ZH' not in fields or 'ZV' not in fields:
                continue
            zh, shp = rows(fields['ZH'])
            zv, _ = rows(fields['ZV'])
            rpb = _block(zh.shape[0], shp[-2], rays_per_block)
            both = ~np.isnan(zh) & ~np.isnan(zv)
            SH, n, N = _sums(zh.astype(np.float64), both, spec, rpb)
            SV, _, _ = _sums(zv.astype(np.float64), both, spec, rpb)
            q, cnt = finish(SH, n, N, np.float32, ratio_of=SV)
        elif k in fields:
            x, shp = rows(fields[k])
            rpb = _block(x.shape[0], shp[-2], rays_per_block)
            S, n, N = _sums(x.astype(np.float64), ~np.isnan(x), spec, rpb)
            q, cnt = finish(S, n, N, np.float64 if k == 'RVEL' else np.float32)
        else:
            continue
        out[k], count[k] = shaped(q, shp), shaped(cnt, shp)
        lead = shp
    if lead is None:
        raise ValueError('average: none of %s in `fields`' % (FIELDS,))
    out['count'] = count
    return out


def coordinates(geom, spec, rays_per_block=0):
    """Window means of the gate coordinates: `geom` {'lats', 'lons', 'dist', 'heights': [n_rays, n_gates]} -> the same names
    [window rows, window columns], float64 (lats, lons) and float32 (dist, heights): the mean over ALL gates of a window
    (a coordinate exists whether or not the gate holds data), by the summation rule of `average`."""
    every = Superob(spec.rays, spec.gates, min_valid_fraction=1.0)
    out = {}
    for k in COORDINATES:
        x = np.asarray(geom[k])
        rpb = _block(x.shape[0], x.shape[0], rays_per_block)
        S, _, N = _sums(x.astype(np.float64), np.ones(x.shape, dtype=bool), every, rpb)
        out[k] = (S / N.astype(np.float64)).astype(x.dtype)
    return out


class Windows(object):
    """The superobservations of ONE sweep call, as RadarOperator._run_rays takes a product ("How a product plugs
    into a sweep call"): `gates` -- the per-gate fields travel to the host too; `refuses` -- the kinds of call it does not
    share; attach / arrays / bind / bind_device / finish / join -- its struct, its arrays and its part of the result."""
    name = 'superob'                      # the entry of the result and of device_outputs
    spectrum, model_var = True, None      # DSPECTRUM travels with the gates; no model variable is integrated for it
    over_members = False                  # (an ensemble call: windows per member, not a reduction over the members)
    refuses = {'groups': 'superobservations need one group'}

    def __init__(self, spec, keep_gates=False, rays_per_block=0, distributed=False):
        # what a superobservation call refuses before it builds anything.  (Spaceborne geometry is refused by the ray calls
        # themselves: they take ground radars.)
        if not isinstance(spec, Superob):
            raise ValueError('superob: a cosmo_pol_amd.superob.Superob, got %r' % (spec,))
        if distributed:
            raise NotImplementedError('superobservations with a process group: the windows would cross the ray shards')
        self.spec, self.gates, self.rays_per_block = spec, bool(keep_gates), rays_per_block

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        n_rays = len(az)
        # (the library refuses the same: the rows of the call are n_members x n_rays, a block never spans two members)
        self.rpb = int(self.rays_per_block) or n_rays
        if int(self.rays_per_block) < 0 or n_rays % self.rpb:
            raise ValueError('rays_per_block %r does not divide the %d rays of the call' % (self.rays_per_block, n_rays))
        self.so = so = native.Superob()
        so.ray_window, so.gate_window, so.rays_per_block = self.spec.rays, self.spec.gates, self.rpb
        so.min_valid_fraction = self.spec.min_valid_fraction
        self.fields = [k for k in FIELDS if k != 'RVEL' or doppler]
        self.wshape = shape(n_rays, n_gates, self.spec, self.rpb)
        if n_members is not None:         # an ensemble call: a leading member axis (the window coordinates come once)
            self.wshape = (n_members,) + self.wshape
        return {'superob': so}, []

    def arrays(self):
        # the window averages, in the sweep's own block: they ride the one copy
        return ([(k, np.float64 if k == 'RVEL' else np.float32, self.wshape) for k in self.fields]
                + [('count', np.uint16, (len(FIELDS),) + self.wshape)])

    def bind(self, path, address):
        setattr(self.so, path, address)

    def bind_device(self, entry):         # {field or 'count': device pointer}
        for k, ptr in entry.items():
            self.bind(k, ptr)

    def finish(self, w, coords):
        cnt = w.pop('count')
        w['count'] = {k: cnt[FIELDS.index(k)] for k in self.fields}
        w.update(coords((self.spec.rays, self.spec.gates, self.rpb), lambda g: coordinates(g, self.spec, self.rpb)))
        return w

    def join(self, parts, cat):
        out = {k: (v if k in COORDINATES else cat([p[k] for p in parts])) for k, v in parts[0].items() if k != 'count'}
        out['count'] = {k: cat([p['count'][k] for p in parts]) for k in parts[0]['count']}
        return out
