"""Time-interpolated scans: the model between two staged states of a forecast series.

Replaces in the reference: nothing -- cosmo_pol reads one model state and simulates every ray at that state's time.
The pure host-side pieces live here so that they are testable without a GPU: the bracket of a ray's time in the
series (which two states, which weight), the host blend of two states that DEFINES what the gate kernel of a timed
sweep computes (k_interp_timed, cpol_members.inl), and the planner that cuts the rays of a call into groups that read
at most as many states as one library call takes.  The operator's entry points are in radar_operator.py.

The blend, per staged variable, element by element, in float32 (a: earlier state, b: later state, w: weight of b):
    w == 0              -> a (b is not read)
    otherwise           -> a + w * (b - a): three float32 operations in that order
    a or b == -9999     -> -9999 (the reference reads a genuine -9999 in variable 0 as a mask code; a blend must not
                           turn the sentinel into an ordinary number)
    NaN                 -> by the formula
The states are blended, not the observables: those are not linear in the state."""
import datetime

import numpy as np

from ._native import MEMBERS_PER_CALL

SENTINEL = np.float32(-9999.0)


def as_seconds(times):
    """Numbers (seconds on any one clock), datetime.datetime or numpy.datetime64 values -> float64 seconds, same shape.
    Datetimes count from 1970-01-01 (naive ones as they stand, aware ones in UTC)."""
    a = np.asarray(times)
    if a.dtype.kind == 'M':
        return a.astype('datetime64[ns]').astype(np.int64) / 1e9
    if a.dtype.kind == 'O':
        def one(d):
            if isinstance(d, datetime.datetime):
                if d.tzinfo is not None:
                    return d.timestamp()
                return (d - datetime.datetime(1970, 1, 1)).total_seconds()
            if isinstance(d, np.datetime64):
                return float(d.astype('datetime64[ns]').astype(np.int64)) / 1e9
            if d is None:
                raise ValueError('a time is None')
            return float(d)
        return np.array([one(d) for d in a.reshape(-1)], dtype=np.float64).reshape(a.shape)
    return a.astype(np.float64)


def check_series(series_times):
    """float64 [n >= 2] times of the series; ValueError naming the first value that does not increase."""
    s = np.asarray(series_times, dtype=np.float64).reshape(-1)
    if len(s) < 2:
        raise ValueError('a series needs at least two states, got %d' % len(s))
    for i in range(len(s)):
        if not np.isfinite(s[i]):
            raise ValueError('series time %d is %r' % (i, s[i]))
        if i and not s[i] > s[i - 1]:
            raise ValueError('series times must increase strictly: time %d (%r) is not after time %d (%r)'
                             % (i, s[i], i - 1, s[i - 1]))
    return s


def bracket(series_times, t):
    """-> (lo, w): int32 index of the earlier state and float32 weight of the later one (lo + 1), in the shape of `t`.
    s[lo] <= t < s[lo + 1] and w = float32((t - s[lo]) / (s[lo + 1] - s[lo])), the quotient taken in float64 and rounded
    once; a time ON a state takes that state with w = 0 (the last time of the series is the only way the last state
    can be `lo`).  A quotient that rounds to 1.0f -- a time within 2^-25 of the bracket's width below the later state --
    takes the later state with w = 0: the weight stays inside [0, 1).  ValueError for a series that does not increase
    strictly and for a time outside it (no extrapolation, no clamping), naming the offending value."""
    s = check_series(series_times)
    tt = np.asarray(t, dtype=np.float64)
    flat = tt.reshape(-1)
    bad = ~((flat >= s[0]) & (flat <= s[-1]))              # (NaN: bad)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError('time %r (entry %d) lies outside the series [%r, %r]' % (flat[i], i, s[0], s[-1]))
    lo = np.searchsorted(s, flat, side='right') - 1        # s[lo] <= t; t == s[-1]: the last state
    w = np.zeros(flat.shape, dtype=np.float32)
    inner = lo < len(s) - 1
    li = lo[inner]
    w[inner] = ((flat[inner] - s[li]) / (s[li + 1] - s[li])).astype(np.float32)
    up = w >= np.float32(1.0)
    lo[up] += 1
    w[up] = 0.0
    return lo.astype(np.int32).reshape(tt.shape), w.reshape(tt.shape)


def blend_states(data_lo, data_hi, w):
    """The host blend of two `data` dicts ({name: [nz, ny, nx]}, as for load_model_arrays) by the rule at the top of
    this module -> a new dict of float32 arrays.  The slow way to a model state between two others, and the definition
    of what a timed sweep computes."""
    w = np.float32(w)
    if not (w >= 0 and w < 1):
        raise ValueError('blend_states: weight %r outside [0, 1)' % (w,))
    if sorted(data_lo) != sorted(data_hi):
        raise ValueError('blend_states: the two states hold different variables (%s)'
                         % ', '.join(sorted(set(data_lo) ^ set(data_hi))))
    out = {}
    for k in data_lo:
        a = np.asarray(data_lo[k], dtype=np.float32)
        if w == 0:
            out[k] = a.copy()                              # (the later state is not read)
            continue
        b = np.asarray(data_hi[k], dtype=np.float32)
        if a.shape != b.shape:
            raise ValueError('blend_states: variable %s has shapes %s and %s' % (k, a.shape, b.shape))
        with np.errstate(invalid='ignore', over='ignore'):
            r = a + w * (b - a)                            # (float32 throughout: three roundings)
        r[(a == SENTINEL) | (b == SENTINEL)] = SENTINEL
        out[k] = r
    return out


def plan_ray_groups(lo, w, max_states=MEMBERS_PER_CALL):
    """Cuts the rays of a timed call into consecutive groups that read at most `max_states` consecutive states each.
    -> [(first ray, end ray, first state, number of states)]: ray r of a group reads state lo[r] - first state of the
    group's list, and the one behind it when w[r] != 0."""
    lo = np.asarray(lo).reshape(-1)
    w = np.asarray(w).reshape(-1)
    if len(lo) and int((lo + (w != 0)).max()) - int(lo.min()) + 1 <= max_states:     # (the usual case: one group)
        return [(0, len(lo), int(lo.min()), int((lo + (w != 0)).max()) - int(lo.min()) + 1)]
    groups = []
    r0, s_min, s_max = 0, None, None
    for r in range(len(lo)):
        a, b = int(lo[r]), int(lo[r]) + (1 if w[r] != 0 else 0)
        if s_min is not None and max(s_max, b) - min(s_min, a) + 1 > max_states:
            groups.append((r0, r, s_min, s_max - s_min + 1))
            r0, s_min, s_max = r, None, None
        s_min = a if s_min is None else min(s_min, a)
        s_max = b if s_max is None else max(s_max, b)
    if s_min is not None:
        groups.append((r0, len(lo), s_min, s_max - s_min + 1))
    return groups
