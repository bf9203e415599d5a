"""Spectrum moments: per gate the power, the mean velocity, the width, skewness and kurtosis, the peak and the edges of the
gate's Doppler spectrum as a call of Doppler scheme 3 delivers it.

Replaces in the reference: nothing -- cosmo_pol forms no moment of the spectrum but RVEL.  The moments are what a user of a
Doppler radar simulation compares with a radar, and they are 64 bytes per gate where the spectrum is 2 KB and more.  The
reduction runs on the device behind the sweep's kernels (k_spec_moments, cpol_spectrum.inl), before the copy to the host; the
pure host-side pieces live here so that they are testable without a GPU: the specification and its refusals, and the NumPy
statement of the rule that DEFINES what the kernel computes (`moments`).  The operator's entry points are in
radar_operator.py.

The rule.  Per gate: the row S[0 .. n_v-1] of DSPECTRUM, float64 -- after the sub-beam accumulation and after the bin-by-bin
sensitivity cut, so censored bins are NaN; the gate-level ZH censoring is not applied, nothing is folded into the Nyquist
interval -- and V[v], the float64 velocity bins.
    a bin counts iff S[v] == S[v] and S[v] > min_power (min_power >= 0, finite, linear units); n = the counting bins
    the ORDERED SUM R[t] of a per-bin term t, float64, every operation one IEEE operation:
        for lane l = 0 .. 63: a_l = +0.0; then for v = l, l + 64, l + 128, ... ascending below n_v, if bin v counts:
        a_l = a_l + t[v]; then for off = 32, 16, 8, 4, 2, 1: every lane at once a_l = a_l + a_(l xor off); R[t] = a_0
    pass 1:  P = R[S];  M = R[V * S] (the product first, then the addition);  vbar = M / P
    pass 2:  per counting bin d = V[v] - vbar, d2 = d * d:  C2 = R[d2 * S];  C3 = R[(d2 * d) * S];  C4 = R[(d2 * d2) * S]
    var = C2 / P;  WIDTH = sqrt(var);  SKEWNESS = (C3 / P) / (var * WIDTH);  KURTOSIS = (C4 / P) / (var * var)
    POWER = P;  VMEAN = vbar;  VPEAK = V[i], i the lowest index among the counting bins that hold the largest S
    VLOW = V[lowest counting index];  VHIGH = V[highest counting index]
    every field is NaN where n < min_bins; count = n always (uint16)
Nothing is special-cased: one counting bin gives WIDTH = 0 and NaN for skewness and kurtosis, overflow gives the inf or NaN
that IEEE gives."""
import numpy as np

# the rows of cpol_spectrum_moments.moments (bit k of `fields`), in this order
FIELDS = ('POWER', 'VMEAN', 'WIDTH', 'SKEWNESS', 'KURTOSIS', 'VPEAK', 'VLOW', 'VHIGH')
LANES = 64
MAX_BINS = 65535


class SpectrumMoments(object):
    """Which moments, of which bins: `fields` out of FIELDS, bins above `min_power` (linear units), NaN where fewer than
    `min_bins` bins count.  ValueError for what the library refuses with CPOL_ERR_ARG: no field or an unknown one,
    min_bins outside 1 ... 65535, min_power negative, NaN or infinite."""

    def __init__(self, fields=('POWER', 'VMEAN', 'WIDTH'), min_power=0.0, min_bins=1):
        if isinstance(fields, str):
            fields = (fields,)
        fields = tuple(fields)
        for k in fields:
            if k not in FIELDS:
                raise ValueError('SpectrumMoments: unknown field %r (known: %s)' % (k, ', '.join(FIELDS)))
        if not fields:
            raise ValueError('SpectrumMoments: no field asked for')
        if int(min_bins) != min_bins:
            raise ValueError('SpectrumMoments: min_bins must be an integer, got %r' % (min_bins,))
        if not 1 <= int(min_bins) <= MAX_BINS:
            raise ValueError('SpectrumMoments: min_bins %r outside 1 ... %d' % (min_bins, MAX_BINS))
        p = float(min_power)
        if not (p >= 0.0 and p != float('inf')):
            raise ValueError('SpectrumMoments: min_power %r must be >= 0 and finite' % (min_power,))
        self.fields = tuple(k for k in FIELDS if k in fields)         # (the order of the rows)
        self.min_power, self.min_bins = p, int(min_bins)

    @property
    def mask(self):
        """cpol_spectrum_moments.fields"""
        return sum(1 << FIELDS.index(k) for k in self.fields)

    @property
    def key(self):
        return (self.fields, self.min_power, self.min_bins)

    def __repr__(self):
        return 'SpectrumMoments(fields=%r, min_power=%r, min_bins=%d)' % self.key


def _ordered_sum(term, counts):
    """R[t]: `term(v)` -> the term of bin v for every gate [n_gates]; counts: bool [n_gates, n_v]"""
    n_gates, n_v = counts.shape
    a = np.zeros((n_gates, LANES), dtype=np.float64)
    for v in range(n_v):
        lane = v % LANES
        a[:, lane] = np.where(counts[:, v], a[:, lane] + term(v), a[:, lane])
    lanes = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lanes ^ off]
    return a[:, 0]


def _rows(spectrum, varray):
    S = np.asarray(spectrum)
    V = np.asarray(varray)
    if S.dtype != np.float64 or V.dtype != np.float64:
        raise ValueError('moments: spectrum and varray are float64')
    if S.ndim < 1 or V.ndim != 1 or S.shape[-1] != V.shape[0] or V.shape[0] < 1:
        raise ValueError('moments: spectrum is [..., n_v], varray [n_v]')
    return np.ascontiguousarray(S).reshape(-1, V.shape[0]), V, S.shape[:-1]


def sums(spectrum, varray, spec):
    """The two passes of the rule: {'counts': bool [n_gates, n_v], 'n', 'P', 'M', 'vbar', 'C2', 'C3', 'C4': [n_gates]} for the
    gates of spectrum [..., n_v], flattened."""
    S, V, _ = _rows(spectrum, varray)
    with np.errstate(all='ignore'):
        counts = (S == S) & (S > spec.min_power)
        n = np.zeros(S.shape[0], dtype=np.int64)
        for v in range(V.shape[0]):
            n = n + counts[:, v]
        P = _ordered_sum(lambda v: S[:, v], counts)
        M = _ordered_sum(lambda v: V[v] * S[:, v], counts)
        vbar = M / P

        def central(power):
            def term(v):
                d = V[v] - vbar
                d2 = d * d
                return (d2 if power == 2 else d2 * d if power == 3 else d2 * d2) * S[:, v]
            return term
        C2, C3, C4 = (_ordered_sum(central(k), counts) for k in (2, 3, 4))
    return {'counts': counts, 'n': n, 'P': P, 'M': M, 'vbar': vbar, 'C2': C2, 'C3': C3, 'C4': C4}


def moments(spectrum, varray, spec):
    """The rule in NumPy: spectrum [..., n_v] float64, varray [n_v] float64, spec a SpectrumMoments ->
    {field: float64 [...] for the fields of `spec`, 'count': uint16 [...]}."""
    S, V, lead = _rows(spectrum, varray)
    r = sums(S, V, spec)
    counts, n, P = r['counts'], r['n'], r['P']
    with np.errstate(all='ignore'):
        var = r['C2'] / P
        width = np.sqrt(var)
        made = {'POWER': P, 'VMEAN': r['vbar'], 'WIDTH': width, 'SKEWNESS': (r['C3'] / P) / (var * width),
                'KURTOSIS': (r['C4'] / P) / (var * var)}
    # the peak and the edges: the lowest index of the largest counting value, the first and the last counting index
    best = np.full(S.shape[0], -1.0)
    i_peak = np.zeros(S.shape[0], dtype=np.int64)
    i_lo = np.full(S.shape[0], -1, dtype=np.int64)
    i_hi = np.zeros(S.shape[0], dtype=np.int64)
    for v in range(V.shape[0]):
        c = counts[:, v]
        better = c & (np.where(c, S[:, v], -1.0) > best)
        best = np.where(better, S[:, v], best)
        i_peak = np.where(better, v, i_peak)
        i_lo = np.where(c & (i_lo < 0), v, i_lo)
        i_hi = np.where(c, v, i_hi)
    made['VPEAK'], made['VLOW'], made['VHIGH'] = V[i_peak], V[np.maximum(i_lo, 0)], V[i_hi]
    few = n < spec.min_bins
    out = {k: np.where(few, np.nan, made[k]).reshape(lead) for k in spec.fields}
    out['count'] = n.astype(np.uint16).reshape(lead)
    return out


class Rows(object):
    """The spectrum moments of ONE sweep call, as RadarOperator._run_rays takes a product ("How a product plugs
    into a sweep call").  `spectrum`: DSPECTRUM travels to the host too (keep_spectrum)."""
    name = 'moments'
    gates, model_var = True, None         # the per-gate fields travel as in the plain call
    refuses = dict.fromkeys(('members', 'timed', 'subbeams'),
                            'spectrum moments are taken by the plain sweeps: no superobservations, ensembles, time blend '
                            'or sub-beam calls')

    def __init__(self, spec, keep_spectrum=False, scheme=3, distributed=False):
        # what a spectrum-moments call refuses before it builds anything
        if not isinstance(spec, SpectrumMoments):
            raise ValueError('moments: a cosmo_pol_amd.spectrum_moments.SpectrumMoments, got %r' % (spec,))
        if scheme != 3:
            raise ValueError('spectrum moments need the Doppler spectrum: doppler scheme 3, configured is %r' % (scheme,))
        if distributed:
            raise NotImplementedError('spectrum moments with a process group: the distributed scans collect no moments')
        self.spec, self.spectrum = spec, bool(keep_spectrum)

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        if not spectrum:                  # (a GPM-type radar: no Doppler whatever the scheme says)
            raise ValueError('spectrum moments need the Doppler spectrum, and this radar simulates none')
        self.sm = native.Context.spectrum_moments_struct(self.spec)
        self.shape = (len(az), n_gates)
        return {'spectrum_moments': self.sm}, []

    def arrays(self):
        # the moments, in the sweep's own block: they ride the one copy (rows nobody asked for arrive as zeros)
        return [('moments', np.float64, (len(FIELDS),) + self.shape), ('count', np.uint16, self.shape)]

    def bind(self, path, address):
        setattr(self.sm, path, address)

    def bind_device(self, entry):         # {'moments': device pointer of [8, n_rays, n_gates], 'count': device pointer}
        for k, ptr in entry.items():
            if k not in ('moments', 'count'):
                raise ValueError("device_outputs['moments']: unknown entry %r" % (k,))
            self.bind(k, ptr)

    def finish(self, w, coords):
        rows = w.pop('moments')
        w.update({k: rows[FIELDS.index(k)] for k in self.spec.fields})
        return w
