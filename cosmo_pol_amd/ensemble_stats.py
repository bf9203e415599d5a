"""Ensemble statistics: per gate the mean, the spread, the extremes of the members of an ensemble, the number of members
that saw an echo and the number of members above thresholds.

Replaces in the reference: nothing -- cosmo_pol runs one model state per process.  A probabilistic forecast or its
verification against observed radar wants none of the members themselves, only these few arrays whose size does not depend
on the number of members.  The fold runs on the device behind the sweeps' kernels (k_member_fold, k_member_finish,
cpol_member_stats.inl), before the copy to the host; the pure host-side pieces live here so that they are testable without a
GPU: the specification and its refusals, and the NumPy statement of the rule that DEFINES what the kernels compute (`fold`,
`finish`, `reduce`).  The operator's entry points are in radar_operator.py.

The rule.  A cell is a gate of the call.  Fields are the ten of superob.FIELDS in that order (ZH, ZV, ZDR, KDP, DELTA_HV,
PHIDP, RHOHV, ATT_H, ATT_V: float32; RVEL: float64; T below).  ZDR is folded from each member's own per-gate ZDR like any
other field: members are not averaged by an antenna, so the power-ratio rule of superobservations does not apply.  mask,
model variables and the Doppler spectrum are not folded.  The state of a pass, per cell and folded field:
    n uint16 = 0;  mean, M2 float64 = +0.0;  lo, hi of type T = +inf, -inf;  k_t uint16 = 0, one per threshold
Members are folded one after another, in the order of the member list.  A member's value v counts iff v == v (a censored or
outside gate is NaN and changes nothing but the member total).  If it counts:
    n = n + 1;  d = float64(v) - mean;  mean = mean + d / float64(n);  M2 = M2 + d * (float64(v) - mean)   (the new mean)
    if v < lo: lo = v;  if v > hi: hi = v;  k_t += (v > thr_t) for each threshold
with the thresholds compared in type T (thr_t: the caller's number rounded once to float32 for the float32 fields) and every
operation one IEEE operation.  Finishing, need = min_members >= 1:
    mean = T(mean) where n >= need, else NaN;  spread = T(sqrt(M2 / float64(n - 1))) where n >= max(need, 2), else NaN (the
    sample standard deviation);  min = lo and max = hi where n >= need, else NaN;  count = n and exceed_t = k_t always
Counts, not probabilities: `probability` divides by the members folded (a NaN reads as "no echo", the right reading of a
censored gate) or by the members that counted.  A strict left fold: the result does not depend on how the member list was
cut into calls.  At most 65535 members per pass and 8 thresholds per field.

Quantiles (EnsembleQuantiles; k_member_quantile on the device).  Per cell and per field with quantiles:
    the counting values of the pass -- the members' values v with v == v, exactly the ones the fold counts, n of them -- are
    ordered ascending by <, with -0.0 before +0.0: a total order on everything that is not NaN, +-inf included.  Sorted they
    are x[0] ... x[n-1].  For a quantile q in [0, 1]: h = q * float64(n - 1), one IEEE multiplication.  One method per pass:
    linear (0): i = floor(h); g = h - float64(i); a = float64(x[i]).  g == 0: a.  Else b = float64(x[i+1]); a == b: a.  Else
                r = a + g * (b - a), three separate float64 operations, then if r > b: r = b.  The quantile is T(r), rounded once.
                An infinite bracket gives what IEEE gives: between -inf and any other value that is NaN, between a finite
                value and +inf it is +inf.
    lower (1): x[floor(h)];  higher (2): x[ceil(h)];  nearest (3): x[rint(h)], ties to even.  These three return a member's own
                bits and make no trip through float64, so they commute with every increasing map (`db`).
    The result is NaN where n < need (min_members, as for the mean).
Because the order is total the quantiles are a symmetric function of the members: they depend neither on the order of the member
list nor on how the pass is cut into calls (unlike the last bits of the mean).  At most 8 quantiles per field, and a pass with
quantiles holds at most 128 members: the device keeps every member of such a field until the pass finishes.

Verification against observations -- the rank of an observed value among the members and the CRPS per gate -- builds on the same
kept members: ensemble_verify.py (EnsembleVerification, a subclass of EnsembleQuantiles; k_member_verify on the device)."""
import numpy as np

# the rows of cpol_member_stats.count, in this order (= superob.FIELDS)
FIELDS = ('ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL')
MAX_MEMBERS = 65535
MAX_THRESHOLDS = 8
MAX_QUANTILES = 8
MAX_QUANTILE_MEMBERS = 128
METHODS = ('linear', 'lower', 'higher', 'nearest')      # cpol_member_stats.quantile_method, in this order
KINDS = ('mean', 'spread', 'min', 'max')
VERIFY_OUTPUTS = ('below', 'equal', 'crps')             # what a verification adds (ensemble_verify.py)


def dtype_of(field):
    return np.float64 if field == 'RVEL' else np.float32


def db(x):
    """10 * log10 of a linear array, computed in float64 and rounded once to the array's own float type: dBZ of ZH and ZV, dB
    of ZDR.  log10 is increasing, and an
    order statistic commutes with an increasing map: the 'lower', 'higher' and 'nearest' quantiles of a linear field ARE the
    quantiles of the field in dB after db() on the result, bit for bit.  'linear' interpolates between two members and does
    not commute (nor do mean and spread)."""
    x = np.asarray(x)
    if x.dtype.kind != 'f':
        x = x.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (10.0 * np.log10(x.astype(np.float64))).astype(x.dtype)


def dbz(x):
    """A reflectivity in dBZ as the linear value the fields carry: 10 ** (x / 10)."""
    return 10.0 ** (np.asarray(x, dtype=np.float64) / 10.0) if np.ndim(x) else 10.0 ** (float(x) / 10.0)


class EnsembleStats(object):
    """What to reduce an ensemble to: `mean`, `spread`, `extremes` (min and max) switch those outputs; `exceed` {field:
    [thresholds in the field's own (linear) units]} asks for the number of members above each; `fields`: the fields to
    fold (None: every field of FIELDS the call produces); `min_members`: mean, min and max are NaN where fewer members
    counted (spread needs two at least).  The count of counting members always comes.  ValueError for what the library
    refuses with CPOL_ERR_ARG: an unknown field, min_members outside 1..65535, more than 8 thresholds for a field, a
    NaN threshold, thresholds for a field that is not folded."""

    def __init__(self, mean=True, spread=True, extremes=False, exceed=None, fields=None, min_members=1):
        self.mean, self.spread, self.extremes = bool(mean), bool(spread), bool(extremes)
        if fields is not None:
            fields = tuple(fields)
            for k in fields:
                if k not in FIELDS:
                    raise ValueError('EnsembleStats: unknown field %r (one of %s)' % (k, FIELDS))
            if not fields or len(set(fields)) != len(fields):
                raise ValueError('EnsembleStats: fields %r is empty or lists a field twice' % (fields,))
            fields = tuple(k for k in FIELDS if k in fields)
        self.fields = fields
        if isinstance(min_members, bool) or int(min_members) != min_members or not 1 <= int(min_members) <= MAX_MEMBERS:
            raise ValueError('EnsembleStats: min_members %r outside 1..%d' % (min_members, MAX_MEMBERS))
        self.min_members = int(min_members)
        self.exceed = {}
        for k, thr in (exceed or {}).items():
            if k not in FIELDS:
                raise ValueError('EnsembleStats: exceed: unknown field %r' % (k,))
            if fields is not None and k not in fields:
                raise ValueError('EnsembleStats: exceed: %r is not among the folded fields %r' % (k, fields))
            thr = np.atleast_1d(np.asarray(thr, dtype=np.float64))
            if thr.ndim != 1 or not 1 <= thr.size <= MAX_THRESHOLDS:
                raise ValueError('EnsembleStats: exceed[%r]: 1 to %d thresholds, got shape %r' % (k, MAX_THRESHOLDS, thr.shape))
            if np.isnan(thr).any():
                raise ValueError('EnsembleStats: exceed[%r]: a threshold is NaN' % (k,))
            self.exceed[k] = thr.copy()

    def resolve(self, available):
        """The fields a call folds, in the order of FIELDS: `fields`, or every field of `available`.  ValueError when a
        requested field (or a field with thresholds) is not available (RVEL without Doppler)."""
        available = [k for k in FIELDS if k in available]
        want = self.fields if self.fields is not None else tuple(available)
        for k in tuple(want) + tuple(self.exceed):
            if k not in available:
                raise ValueError('EnsembleStats: field %r is not produced by this call (RVEL needs a Doppler scheme)' % (k,))
        if not want:
            raise ValueError('EnsembleStats: no field to fold')
        return tuple(want)

    def thresholds(self, field):
        """The thresholds of `field` as the fold compares them: rounded once to the field's dtype."""
        return self.exceed.get(field, np.zeros(0)).astype(dtype_of(field))

    @property
    def kinds(self):
        return tuple(k for k, on in zip(KINDS, (self.mean, self.spread, self.extremes, self.extremes)) if on)

    @property
    def key(self):
        return (self.mean, self.spread, self.extremes, self.fields, self.min_members,
                tuple((k, tuple(v)) for k, v in sorted(self.exceed.items())))

    def __repr__(self):
        return 'EnsembleStats(mean=%r, spread=%r, extremes=%r, exceed=%r, fields=%r, min_members=%d)' % (
            self.mean, self.spread, self.extremes, {k: list(v) for k, v in self.exceed.items()}, self.fields, self.min_members)


class EnsembleQuantiles(EnsembleStats):
    """EnsembleStats plus QUANTILES of the members per gate: `quantiles` {field: [q, ...]} (a scalar is accepted), each q in
    [0, 1], at most 8 per field; `method`: 'linear' (the default), 'lower', 'higher' or 'nearest', one for the pass (the rule
    at the top of this module).  The other keywords are those of EnsembleStats.  The result gains 'quantile': {field: array
    [n_q, ...cells] in the field's type}.  A pass with quantiles holds at most 128 members.  ValueError for an unknown field,
    a field outside `fields`, 0 or more than 8 values for a field, a q that is NaN or outside [0, 1], an unknown method."""

    def __init__(self, quantiles, method='linear', **kw):
        EnsembleStats.__init__(self, **kw)
        if method not in METHODS:
            raise ValueError('EnsembleQuantiles: method %r (one of %s)' % (method, METHODS))
        self.method = method
        if not isinstance(quantiles, dict):
            raise ValueError('EnsembleQuantiles: quantiles is {field: [q, ...]}, got %r' % (quantiles,))
        self.quantiles = {}
        for k, q in quantiles.items():
            if k not in FIELDS:
                raise ValueError('EnsembleQuantiles: quantiles: unknown field %r' % (k,))
            if self.fields is not None and k not in self.fields:
                raise ValueError('EnsembleQuantiles: quantiles: %r is not among the folded fields %r' % (k, self.fields))
            q = np.atleast_1d(np.asarray(q, dtype=np.float64))
            if q.ndim != 1 or not 1 <= q.size <= MAX_QUANTILES:
                raise ValueError('EnsembleQuantiles: quantiles[%r]: 1 to %d values, got shape %r' % (k, MAX_QUANTILES, q.shape))
            if not np.all((q >= 0.0) & (q <= 1.0)):         # (false for NaN)
                raise ValueError('EnsembleQuantiles: quantiles[%r]: every q lies in [0, 1], got %r' % (k, list(q)))
            self.quantiles[k] = q.copy()

    @classmethod
    def median(cls, fields=None, **kw):
        """The median (q = 0.5) of `fields` (None: of the fields of the `fields` keyword, or of every field of FIELDS but
        RVEL, which needs a Doppler scheme)."""
        if fields is None:
            fields = kw.get('fields') or FIELDS[:-1]
        return cls({k: [0.5] for k in fields}, **kw)

    def resolve(self, available):
        names = EnsembleStats.resolve(self, available)
        for k in self.quantiles:
            if k not in names:
                raise ValueError('EnsembleQuantiles: field %r is not produced by this call (RVEL needs a Doppler scheme)' % (k,))
        return names

    @property
    def key(self):
        return EnsembleStats.key.fget(self) + (self.method, tuple((k, tuple(v)) for k, v in sorted(self.quantiles.items())))

    def __repr__(self):
        return 'EnsembleQuantiles(quantiles=%r, method=%r, mean=%r, spread=%r, extremes=%r, exceed=%r, fields=%r, min_members=%d)' % (
            {k: list(v) for k, v in self.quantiles.items()}, self.method, self.mean, self.spread, self.extremes,
            {k: list(v) for k, v in self.exceed.items()}, self.fields, self.min_members)


def _quantiles_of(spec):
    return getattr(spec, 'quantiles', None) or {}


def order_key(x):
    """The monotone integer key of the rule's order: the bits of a negative value flipped, the sign bit of a non-negative one
    set -- -0.0 comes before +0.0.  NaN gets the largest key (no other value has it)."""
    x = np.asarray(x)
    U = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
    u = x.view(U)
    sign = U(1) << U(8 * x.dtype.itemsize - 1)
    key = np.where(u & sign != 0, ~u, u | sign)
    return np.where(x != x, ~U(0), key)


def quantiles(x, q, method='linear', need=1):
    """The rule's quantiles `q` of the members x [n_members, ...cells] (float32 or float64) -> [len(q), ...cells] in x's type."""
    x = np.asarray(x)
    T = x.dtype.type
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    cells = x.shape[1:]
    out = np.full((len(q),) + cells, np.nan, T)
    if x.shape[0] == 0:
        return out
    order = np.argsort(order_key(x), axis=0, kind='stable')       # (NaNs last; equal keys are equal bits)
    xs = np.take_along_axis(x, order, axis=0)
    n = np.sum(x == x, axis=0).astype(np.int64)
    top = np.maximum(n - 1, 0)

    def at(i):
        return np.take_along_axis(xs, np.minimum(i, top)[None], axis=0)[0]

    with np.errstate(all='ignore'):
        for t, qt in enumerate(q):
            h = qt * (n - 1).astype(np.float64)
            if method == 'linear':
                i = np.floor(h)
                g = h - i
                i = i.astype(np.int64)
                a, b = at(i).astype(np.float64), at(i + 1).astype(np.float64)
                d = b - a
                r = a + g * d
                r = np.where(r > b, b, r)
                r = np.where((g == 0.0) | (a == b), a, r).astype(T)
            elif method == 'lower':
                r = at(np.floor(h).astype(np.int64))
            elif method == 'higher':
                r = at(np.ceil(h).astype(np.int64))
            elif method == 'nearest':
                r = at(np.rint(h).astype(np.int64))
            else:
                raise ValueError('quantiles: method %r (one of %s)' % (method, METHODS))
            out[t] = np.where(n >= need, r, T(np.nan))
    return out


def begin(spec, fields, shape):
    """The state of a pass that has folded nothing: {'spec', 'n_members', 'fields': {name: {'n', 'mean', 'M2', 'lo', 'hi',
    'k'}}} for cells of `shape`; a field with quantiles (or a verification) also keeps its members, 'x': the rows in fold order."""
    shape = tuple(shape)
    st = {}
    for k in fields:
        T = dtype_of(k)
        thr = spec.thresholds(k)
        st[k] = {'n': np.zeros(shape, np.uint16), 'mean': np.zeros(shape, np.float64), 'M2': np.zeros(shape, np.float64),
                 'lo': np.full(shape, np.inf, T), 'hi': np.full(shape, -np.inf, T),
                 'k': np.zeros((len(thr),) + shape, np.uint16), 'thr': thr}
        if k in _quantiles_of(spec) or k in getattr(spec, 'verify', ()):      # (ensemble_verify: a verified field keeps them too)
            st[k]['x'] = np.zeros((0,) + shape, T)
    return {'spec': spec, 'n_members': 0, 'fields': st}


def fold(state, rows):
    """Folds the members of `rows` {name: [n_members, ...cells]} into `state`, one after another: the rule at the top of this
    module in NumPy, statement by statement.  Returns `state`."""
    n_new = None
    for name, s in state['fields'].items():
        T = dtype_of(name)
        x = np.asarray(rows[name])
        if x.dtype != T or x.shape[1:] != s['n'].shape:
            raise ValueError('fold: %s must be %s [n_members%s], got %s %r'
                             % (name, np.dtype(T).name, ''.join(', %d' % d for d in s['n'].shape), x.dtype, x.shape))
        if n_new is not None and x.shape[0] != n_new:
            raise ValueError('fold: the fields hold different numbers of members')
        n_new = x.shape[0]
        if state['n_members'] + n_new > MAX_MEMBERS:
            raise ValueError('fold: more than %d members in a pass' % MAX_MEMBERS)
        if 'x' in s:
            if state['n_members'] + n_new > MAX_QUANTILE_MEMBERS:
                raise ValueError('fold: more than %d members in a pass with quantiles' % MAX_QUANTILE_MEMBERS)
            s['x'] = np.concatenate([s['x'], x])
        n, mean, M2, lo, hi, k = s['n'], s['mean'], s['M2'], s['lo'], s['hi'], s['k']
        with np.errstate(all='ignore'):
            for v in x:
                c = v == v
                v64 = v.astype(np.float64)
                n = (n + c).astype(np.uint16)
                d = v64 - mean
                new = mean + d / n.astype(np.float64)
                M2 = np.where(c, M2 + d * (v64 - new), M2)
                mean = np.where(c, new, mean)
                lo = np.where(c & (v < lo), v, lo)
                hi = np.where(c & (v > hi), v, hi)
                for t, thr in enumerate(s['thr']):
                    k[t] = k[t] + (c & (v > thr))
        s.update(n=n, mean=mean, M2=M2, lo=lo, hi=hi)
    state['n_members'] += n_new or 0
    return state


def finish(state, spec=None):
    """The outputs of a pass: {'mean', 'spread', 'min', 'max': {name: array in the field's dtype} (those `spec` asks for),
    'count': {name: uint16}, 'exceed': {name: uint16 [n_thresholds, ...cells]}, 'n_members'}, and 'quantile': {name: [n_q,
    ...cells] in the field's dtype} when `spec` asks for quantiles."""
    spec = spec or state['spec']
    need = spec.min_members
    out = {kind: {} for kind in spec.kinds}
    out.update(count={}, exceed={}, n_members=state['n_members'])
    if _quantiles_of(spec):
        out['quantile'] = {}
    for name, s in state['fields'].items():
        T = dtype_of(name)
        n = s['n'].astype(np.int64)
        nan = np.array(np.nan, T)
        if spec.mean:
            out['mean'][name] = np.where(n >= need, s['mean'].astype(T), nan)
        if spec.spread:
            with np.errstate(all='ignore'):
                sd = np.sqrt(s['M2'] / (n - 1).astype(np.float64)).astype(T)
            out['spread'][name] = np.where(n >= max(need, 2), sd, nan)
        if spec.extremes:
            out['min'][name] = np.where(n >= need, s['lo'], nan)
            out['max'][name] = np.where(n >= need, s['hi'], nan)
        out['count'][name] = s['n'].copy()
        if len(s['thr']):
            out['exceed'][name] = s['k'].copy()
        if name in _quantiles_of(spec):
            out['quantile'][name] = quantiles(s['x'], spec.quantiles[name], spec.method, need)
    return out


def reduce(fields, spec):
    """`fields` {name: [n_members, ...cells]} as simulate_rays_ensemble returns them (other entries are ignored) -> the
    statistics of `finish`: the slow way to them, and the definition of what the device computes."""
    have = [k for k in FIELDS if k in fields]
    names = spec.resolve(have)
    rows = {k: np.asarray(fields[k]) for k in names}
    return finish(fold(begin(spec, names, rows[names[0]].shape[1:]), rows), spec)


def probability(stats, field, of='members'):
    """exceed / n_members (of='members': a member without an echo counts as below every threshold) or exceed / count
    (of='valid': among the members that counted; NaN where none did) -> float64 [n_thresholds, ...cells]."""
    if of not in ('members', 'valid'):
        raise ValueError("probability: of is 'members' or 'valid'")
    k = stats['exceed'][field].astype(np.float64)
    if of == 'members':
        if stats['n_members'] < 1:
            raise ValueError('probability: no member was folded')
        return k / float(stats['n_members'])
    with np.errstate(invalid='ignore', divide='ignore'):
        return k / stats['count'][field].astype(np.float64)


class Fold(object):
    """The ensemble statistics -- quantiles and verification with them: one struct pair, one pass -- of ONE sweep call, as
    RadarOperator._run_rays takes a product ("How a product plugs into a sweep call"): this call's member(s) folded
    into the lane's running statistics.  `phase` is set anew for every call of a pass (bit 0 begins it, bit 1 finishes it: the
    statistics arrive with that call); `capacity`: the members of the whole pass; `observations`: the finishing call's, for a
    verification ({field: [n_rays, n_gates]}, as ensemble_verify.check_observations hands them back)."""
    name = 'stats'
    spectrum, model_var = True, None
    over_members = True                   # (an ensemble call: its chunks form one pass, and only the last holds the result)
    refuses = dict.fromkeys(('timed', 'subbeams'),
                            'ensemble statistics are taken by the ensemble sweeps, not by time-blended or sub-beam calls')

    def __init__(self, spec, keep_members=False, phase=3, capacity=None, observations=None):
        self.quantiles = getattr(spec, 'quantiles', None) or {}
        self.verify = getattr(spec, 'verify', None) or ()
        n = capacity or 0
        # (before anything runs: the device keeps every member of a field with quantiles, and likewise of a verified field,
        # until the pass finishes)
        if self.quantiles and n > MAX_QUANTILE_MEMBERS:
            raise ValueError('ensemble quantiles: at most %d members in a pass' % MAX_QUANTILE_MEMBERS)
        if self.verify and n > MAX_QUANTILE_MEMBERS:
            raise ValueError('ensemble verification: at most %d members in a pass' % MAX_QUANTILE_MEMBERS)
        if n > MAX_MEMBERS:
            raise ValueError('ensemble statistics: at most %d members in a pass' % MAX_MEMBERS)
        self.spec, self.gates, self.phase, self.capacity, self.observations = spec, bool(keep_members), int(phase), capacity, observations

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        self.names = self.spec.resolve([k for k in FIELDS if k != 'RVEL' or doppler])
        self.ms, keep = native.Context.member_stats_struct(self.spec, self.names, self.phase, capacity=self.capacity)
        structs = {'member_stats': self.ms}
        self.gshape = (len(az), n_gates)          # (per gate, whatever the number of members)
        if self.verify:                           # (fields and fair go with every call of the pass)
            self.mv = structs['member_verify'] = native.Context.member_verify_struct(self.spec)
            if self.phase & 2 and take is not None:
                # ... and the observations in a page-locked block of their own, which the device reads in place.  (A clean
                # block: no writer is named, so none whose last copy may still be in flight -- the host writes it now.)
                views, addresses = take([(k, dtype_of(k), self.gshape) for k in self.verify])
                for k, v, a in zip(self.verify, views, addresses):
                    v[...] = self.observations[k]
                    self.bind(('obs', k), a)
                keep = keep + views               # (the block: k_member_verify reads it until this call is done)
        return structs, keep

    def arrays(self):
        # the statistics, in the sweep's own block: they ride the one copy
        if not self.phase & 2:
            return []
        spec, names, g = self.spec, self.names, self.gshape
        out = [((kind, k), dtype_of(k), g) for kind in spec.kinds for k in names]
        out.append(('count', np.uint16, (len(FIELDS),) + g))
        out += [(('exceed', k), np.uint16, (len(spec.exceed[k]),) + g) for k in names if k in spec.exceed]
        out += [(('quantile', k), dtype_of(k), (len(self.quantiles[k]),) + g) for k in names if k in self.quantiles]
        for k in self.verify:
            out += [(('below', k), np.uint16, g), (('equal', k), np.uint16, g), (('crps', k), dtype_of(k), g)]
        return out

    def bind(self, path, address):
        if path == 'count':
            self.ms.count = address
        else:                             # (the verification: observations in, ranks and CRPS out -- the second struct)
            kind, k = path
            getattr(self.mv if kind in ('obs',) + VERIFY_OUTPUTS else self.ms, kind)[FIELDS.index(k)] = address

    def bind_device(self, entry):
        # {'mean' | 'spread' | 'min' | 'max' | 'exceed' | 'quantile': {field: device pointer}, 'count': pointer}; with a
        # verification also 'obs' | 'below' | 'equal' | 'crps': {field: device pointer}
        for kind, ptrs in (entry.items() if self.phase & 2 else ()):
            if kind == 'count':
                self.bind(kind, ptrs)
                continue
            if kind in ('obs',) + VERIFY_OUTPUTS:
                if not self.verify:
                    raise ValueError("device_outputs['stats'][%r] without an EnsembleVerification" % (kind,))
            elif kind not in KINDS + ('exceed', 'quantile'):
                raise ValueError("device_outputs['stats']: unknown entry %r" % (kind,))
            for k, ptr in ptrs.items():
                self.bind((kind, k), ptr)

    def finish(self, views, coords):
        cnt = views.pop('count')
        w = {}
        for (kind, k), a in views.items():
            (w.setdefault('verify', {}) if kind in VERIFY_OUTPUTS else w).setdefault(kind, {})[k] = a
        w['count'] = {k: cnt[FIELDS.index(k)] for k in self.names}
        w.setdefault('exceed', {})
        if self.quantiles:
            w.setdefault('quantile', {})
        if self.capacity is not None:
            w['n_members'] = self.capacity
        return w

    def join(self, parts, cat):
        return parts[-1]                  # (one pass: the finishing call holds the statistics)
