"""Ensemble verification: the members of an ensemble scored against an observed sweep, per gate -- the rank of the observation
among the members and the CRPS -- plus the host helpers that turn the per-gate arrays into a rank histogram and a Brier score.

Replaces in the reference: nothing -- cosmo_pol runs one model state per process.  The scores are formed on the device behind the
pass of ensemble statistics (k_member_verify, cpol_member_stats.inl: the stash of k_member_fold holds every member of a verified
field when the pass finishes), before the copy to the host; the pure host-side pieces live here so that they are testable
without a GPU: the specification and its refusals, and the NumPy statement of the rule that DEFINES what the kernel computes
(`verify`, `reduce`).  The operator's entry points are in radar_operator.py (simulate_rays_ensemble_stats(..., observations=)).

The rule (the same text stands in include/cosmo_pol_amd.h).  A cell is a gate of the call.  A verified field k is one of the ten
of ensemble_stats.FIELDS; its type T is float32, except RVEL, which is float64.  Each verified field has an observation array
obs[k] of n_cells values of type T.  The observation y = obs[k][c] is in the field's own (linear) units.  NaN means no observation.
The counting members of the pass are exactly the ones the fold counts (v == v, n of them).  They are ordered by the total order
of the quantile rule (ensemble_stats.order_key, `key` below: -0.0 before +0.0, +-inf included).  Sorted, they are x[0] ... x[n-1].
Ranks:
    below = the number of i with key(x[i]) < key(y);  equal = the number of i with key(x[i]) == key(y).  Both uint16, both
    written always, like `count`, and both 0 where y is NaN.  min_members does not gate them.
CRPS (type T):
    NaN where y is NaN; NaN where n < need (min_members); NaN where n == 0; with `fair`, NaN where n < 2.  Otherwise in float64,
    every operation one IEEE operation, with no contraction and no reciprocal:
        yd = float64(y)
        A = +0.0;  for i = 0 ... n-1 ascending: A = A + fabs(float64(x[i]) - yd)
        B = +0.0;  for i = 0 ... n-1 ascending: B = B + float64(2*i - n + 1) * float64(x[i])   (the product first, then added)
        D = n*n, or n*(n-1) when `fair` (a whole number of at most 16384)
        r = A / float64(n) - B / float64(D)   (each quotient rounded once, subnormal quotients too)
        if r < 0: r = +0.0;  crps = T(r)
    This is (1/n) sum |x_i - y| - (1/2D) sum_i sum_j |x_i - x_j|: the double sum over ordered pairs is 2B for a sorted sample.
    Infinite members or observations are not special-cased: IEEE decides.
The sums run over the sorted values, so all three outputs are symmetric functions of the members: they depend neither on the order
of the member list nor on how the pass is cut into calls.  A pass with a verified field holds at most 128 members (the device
keeps every member of such a field until the pass finishes, like a field with quantiles).

Not built: CRPS in dB, reductions across gates on the device (the helpers below run on the host), verification of
superobservation windows and of time-blended sweeps."""
import numpy as np

from . import ensemble_stats as ES

FIELDS = ES.FIELDS
MAX_MEMBERS = ES.MAX_QUANTILE_MEMBERS
OUTPUTS = ES.VERIFY_OUTPUTS


class EnsembleVerification(ES.EnsembleQuantiles):
    """EnsembleQuantiles plus the VERIFICATION of `verify` (field names) against observations: the result gains 'verify':
    {'below' | 'equal': {field: uint16 array}, 'crps': {field: array in the field's type}}.  `fair`: the pair term of the CRPS
    is divided by n (n - 1) instead of n n (the score of the underlying distribution rather than of the n members).
    `quantiles` ({field: [q, ...]}) may be empty or None; the other keywords are those of EnsembleQuantiles / EnsembleStats.
    ValueError for an unknown or duplicate field, a verified field outside `fields`, a `fair` that is not a bool."""

    def __init__(self, verify=('ZH',), fair=False, quantiles=None, **kw):
        ES.EnsembleQuantiles.__init__(self, quantiles or {}, **kw)
        if isinstance(verify, str):
            verify = (verify,)
        verify = tuple(verify)
        for k in verify:
            if k not in FIELDS:
                raise ValueError('EnsembleVerification: verify: unknown field %r (one of %s)' % (k, FIELDS))
            if self.fields is not None and k not in self.fields:
                raise ValueError('EnsembleVerification: verify: %r is not among the folded fields %r' % (k, self.fields))
        if not verify or len(set(verify)) != len(verify):
            raise ValueError('EnsembleVerification: verify %r is empty or lists a field twice' % (verify,))
        if not isinstance(fair, (bool, np.bool_)):
            raise ValueError('EnsembleVerification: fair is True or False, got %r' % (fair,))
        self.verify = tuple(k for k in FIELDS if k in verify)
        self.fair = bool(fair)

    def resolve(self, available):
        names = ES.EnsembleQuantiles.resolve(self, available)
        for k in self.verify:
            if k not in names:
                raise ValueError('EnsembleVerification: field %r is not produced by this call (RVEL needs a Doppler scheme)' % (k,))
        return names

    @property
    def key(self):
        return ES.EnsembleQuantiles.key.fget(self) + (self.verify, self.fair)

    def __repr__(self):
        return 'EnsembleVerification(verify=%r, fair=%r, quantiles=%r, method=%r, mean=%r, spread=%r, extremes=%r, exceed=%r, fields=%r, min_members=%d)' % (
            self.verify, self.fair, {k: list(v) for k, v in self.quantiles.items()}, self.method, self.mean, self.spread,
            self.extremes, {k: list(v) for k, v in self.exceed.items()}, self.fields, self.min_members)


def check_observations(spec, names, observations, shape):
    """{field: array} of the verified fields among `names`, each of the field's dtype and of `shape`, C-contiguous.  ValueError
    for a missing verified field, a wrong dtype or shape."""
    if not isinstance(observations, dict):
        raise ValueError('observations: {field: array}, got %r' % (type(observations),))
    out = {}
    for k in spec.verify:
        if k not in names:
            raise ValueError('observations: the verified field %r is not folded by this call' % (k,))
        if k not in observations:
            raise ValueError('observations: the verified field %r has none' % (k,))
        a = np.asarray(observations[k])
        if a.dtype != ES.dtype_of(k) or a.shape != tuple(shape):
            raise ValueError('observations[%r] must be %s %r, got %s %r' % (k, np.dtype(ES.dtype_of(k)).name, tuple(shape), a.dtype, a.shape))
        out[k] = np.ascontiguousarray(a)
    return out


def verify(x, y, need=1, fair=False):
    """The rule on the members x [n_members, ...cells] and the observations y [...cells] (both float32 or both float64) ->
    {'below', 'equal': uint16 [...cells], 'crps': [...cells] in x's type}: NumPy, statement by statement."""
    v = unrounded(x, y, fair)
    T = np.asarray(x).dtype.type
    n = v['n']
    ok = (v['y'] == v['y']) & (n >= need) & (n > 0) & ((n >= 2) if fair else True)
    with np.errstate(all='ignore'):
        crps = np.where(ok, v['r'].astype(T), T(np.nan))
    return {'below': v['below'], 'equal': v['equal'], 'crps': crps}


def unrounded(x, y, fair=False):
    """The rule up to its last two steps: {'n': int64, 'below', 'equal': uint16, 'r': float64 -- the score after the clamp and
    before the rounding to the field's type, whatever n and y are (NaN or meaningless where the CRPS is NaN) --, 'y'}."""
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype != y.dtype or x.dtype.kind != 'f' or x.dtype.itemsize not in (4, 8) or x.shape[1:] != y.shape:
        raise ValueError('verify: x [n_members, ...cells] and y [...cells] of one float type, got %s %r and %s %r'
                         % (x.dtype, x.shape, y.dtype, y.shape))
    if x.shape[0] > MAX_MEMBERS:
        raise ValueError('verify: more than %d members' % MAX_MEMBERS)
    M = x.shape[0]
    kx = ES.order_key(x)                                    # (NaN: the largest key)
    order = np.argsort(kx, axis=0, kind='stable')           # (NaNs last; equal keys are equal bits)
    xs = np.take_along_axis(x, order, axis=0)
    ks = np.take_along_axis(kx, order, axis=0)
    n = np.sum(x == x, axis=0).astype(np.int64)
    seen = y == y
    ky = ES.order_key(y)
    below = np.zeros(y.shape, np.int64)
    equal = np.zeros(y.shape, np.int64)
    for i in range(M):
        counts = (i < n) & seen
        below = below + (counts & (ks[i] < ky))
        equal = equal + (counts & (ks[i] == ky))
    with np.errstate(all='ignore'):
        yd = y.astype(np.float64)
        A = np.zeros(y.shape, np.float64)
        for i in range(M):
            A = np.where(i < n, A + np.fabs(xs[i].astype(np.float64) - yd), A)
        B = np.zeros(y.shape, np.float64)
        for i in range(M):
            p = (2 * i - n + 1).astype(np.float64) * xs[i].astype(np.float64)
            B = np.where(i < n, B + p, B)
        D = n * (n - 1) if fair else n * n
        r = A / n.astype(np.float64) - B / D.astype(np.float64)
        r = np.where(r < 0, 0.0, r)
    return {'n': n, 'below': below.astype(np.uint16), 'equal': equal.astype(np.uint16), 'r': r, 'y': y}


def finish(state, observations, spec=None):
    """ensemble_stats.finish plus 'verify' for the state of a pass begun with an EnsembleVerification (ensemble_stats.begin /
    fold keep the members of its verified fields)."""
    spec = spec or state['spec']
    out = ES.finish(state, spec)
    shape = next(iter(state['fields'].values()))['n'].shape
    obs = check_observations(spec, list(state['fields']), observations, shape)
    out['verify'] = {k: {} for k in OUTPUTS}
    for name in spec.verify:
        v = verify(state['fields'][name]['x'], obs[name], spec.min_members, spec.fair)
        for k in OUTPUTS:
            out['verify'][k][name] = v[k]
    return out


def reduce(fields, observations, spec):
    """`fields` {name: [n_members, ...cells]} as simulate_rays_ensemble returns them, `observations` {name: [...cells]} -> the
    statistics of ensemble_stats.reduce plus 'verify': {'below' | 'equal' | 'crps': {field: array}}: the slow way to them, and
    the definition of what the device computes."""
    have = [k for k in FIELDS if k in fields]
    names = spec.resolve(have)
    rows = {k: np.asarray(fields[k]) for k in names}
    return finish(ES.fold(ES.begin(spec, names, rows[names[0]].shape[1:]), rows), observations, spec)


def rank_histogram(below, equal, count, n_members, ties='split', present=None):
    """The rank histogram [n_members + 1] (float64) over the gates where every member counted (count == n_members) and the
    observation is present.  `present`: a boolean array, e.g. ~np.isnan(observation) or ~np.isnan(crps) -- the ranks alone do
    not tell a missing observation (below = equal = 0) from one below every member; None: every gate has one.  The
    observation's rank lies in below ... below + equal.  ties='split': the gate's one count is spread evenly over those
    equal + 1 bins, as float64 counts; 'low': all of it into bin `below`; 'high': into bin below + equal."""
    if ties not in ('split', 'low', 'high'):
        raise ValueError("rank_histogram: ties is 'split', 'low' or 'high'")
    n_members = int(n_members)
    if n_members < 1:
        raise ValueError('rank_histogram: n_members >= 1')
    below, equal, count = (np.asarray(a).astype(np.int64).reshape(-1) for a in (below, equal, count))
    if not below.shape == equal.shape == count.shape:
        raise ValueError('rank_histogram: below, equal and count have one shape')
    use = count == n_members
    if present is not None:
        present = np.asarray(present, dtype=bool).reshape(-1)
        if present.shape != use.shape:
            raise ValueError('rank_histogram: present has the shape of below')
        use = use & present
    b, e = below[use], equal[use]
    if ((b < 0) | (e < 0) | (b + e > n_members)).any():
        raise ValueError('rank_histogram: below + equal exceeds n_members')
    hist = np.zeros(n_members + 1, np.float64)
    if ties == 'low':
        np.add.at(hist, b, 1.0)
    elif ties == 'high':
        np.add.at(hist, b + e, 1.0)
    else:
        w = 1.0 / (e + 1).astype(np.float64)
        for j in range(int(e.max()) + 1 if e.size else 0):
            sel = e >= j
            np.add.at(hist, b[sel] + j, w[sel])
    return hist


def brier(stats, observed, field, thresholds):
    """The Brier score of the exceedance probabilities of `field`, per threshold -> float64 [n_thresholds]: the mean over the
    gates with an observation (observed == observed) of (p - o) ** 2, p = stats['exceed'][field] / stats['n_members'] (a member
    without an echo counts as below every threshold, ensemble_stats.probability of='members') and o = observed > threshold.
    `thresholds`: the spec the statistics were made under (its thresholds as the fold compares them) or the numbers themselves.
    NaN where no gate has an observation."""
    if isinstance(thresholds, ES.EnsembleStats):
        thr = thresholds.thresholds(field)
    else:
        thr = np.atleast_1d(np.asarray(thresholds)).astype(ES.dtype_of(field))
    p = ES.probability(stats, field, of='members')
    observed = np.asarray(observed)
    if p.shape != (len(thr),) + observed.shape:
        raise ValueError('brier: exceed[%r] is %r, observed %r, %d threshold(s)' % (field, p.shape, observed.shape, len(thr)))
    seen = observed == observed
    out = np.full(len(thr), np.nan)
    if seen.any():
        for t in range(len(thr)):
            o = (observed[seen] > thr[t]).astype(np.float64)
            out[t] = np.mean((p[t][seen] - o) ** 2)
    return out
