"""Object cells (cpol_objects): the connected components of the binary maps of a neighbourhood verification, numbered, with ten
integer attributes each and, when asked for, the EXACT float sums over their cells (rain volume, weighted moments), found on the
device behind the scores.  This module states the rule in NumPy (`cells`, `exact_sum`, `weight_of`); include/cosmo_pol_amd.h
states the same text, and the GPU tests compare the kernels (cosmo_pol_amd/csrc/cpol_obj.inl) with it exactly: every attribute
is a count, an integer sum, an integer extreme or a comparison, and every float sum is a sum of integers rounded once.

THE RULE
  Input      the binary maps of neighbourhood.Fractions, unchanged: F[b, t] = domain & (m == m) & (m >= thr[t]) of the scored
             plane's blocks, O[t] likewise of the observed map; float32 comparisons, thresholds rounded once.
  Sources    one map per source s and threshold t: sources 0 ... n_blocks - 1 are the blocks, source n_blocks is the observed map.
  Object     a maximal set of set cells connected through `connectivity` neighbours: 4 (edges) or 8 (edges and corners).
  First cell the cell of an object with the smallest flat index iy * n_x + ix.
  Filter     objects with fewer than `min_area` (>= 1) cells are dropped.
  Numbering  the kept objects are numbered 1 ... n in ascending order of their first cell: scipy.ndimage.label's numbering when
             min_area = 1.
  Attributes WORDS = 10 uint32 per kept object: first, area, sum of ix, sum of iy, the inclusive bounding box x0, x1, y0, y1,
             peak_cell, the float32 bits of the peak value.  The peak is the largest value of the object's cells in the total
             order of float32, in which -0.0 lies before +0.0 (among the two the peak is +0.0 wherever it lies); among cells of
             equal bits the one with the smallest flat index.
  Overflow   none is possible: at most 1023 x 1023 cells, so an area is < 2^20 and a sum of ix < 2^30.
  Outputs    n_objects uint32 [n_blocks + 1, n_thr]: the true kept count, also beyond max_objects; table uint32 [n_blocks + 1,
             n_thr, max_objects, WORDS], rows at or beyond n_objects zero; labels int32 [n_blocks + 1, n_thr, n_y, n_x], 0 for
             background and dropped objects, complete even when the table overflows.  `result` names them.
  Limits     the labelling scratch, (n_blocks + 1) * n_thr * (2 * n_y * n_x + n_y) * 4 bytes, at most MAX_SCRATCH_BYTES.

EXACT SUMS (Objects(sums=True); `weighted_centroids` and `sal` read them)
  Summand    for a cell with plane value m (o for the observed map) the summand is w = m.  With a weight table (table_v float32
             strictly ascending, table_f float64) it is w = float32(f(m)), f the piecewise-linear function that
             composite.column_of evaluates, statement by statement: searchsorted(..., 'right') - 1; t = (m - v_i) / (v_i+1 - v_i),
             d, p = t * d, f_i + p, each one float64 operation; 0 below the table, table_f[-1] at and above its end; then one
             rounding to float32 (`weight_of`).  table_f must be finite and non-decreasing, so that the peak of w is w(peak):
             SAL on rain rate under a Z-R table (`zr_table`) instead of linear Z.
  Skipped    a cell whose w is +-inf is not summed; it is counted in `skipped`.  NaN cells are never set.
  Per object with a table row: volume = sum w, moment_x = sum w * ix, moment_y = sum w * iy over its cells, each sum formed
             exactly (a float32 is an integer multiple of 2^-149, a product w * ix is exact: 24 + 10 bits) and rounded ONCE to
             float64, round-to-nearest-even: math.fsum of the summands, whatever their order.  An exact zero is +0.0.
  Per source independent of the threshold: the same three sums over every cell with domain && m == m, and the cells summed and
             skipped.
  The rule   `exact_sum`: integers alone.  The bits of a float32 are sign, E = max(e, 1) and a 24-bit M: the value is
             +-M * 2^(E - 150).  The integers M << E (times ix) are added and the total rounded by hand.
  Outputs    volume float64 [n_blocks + 1, n_thr, max_objects, 3], rows at or beyond n_objects zero; skipped uint32 [n_blocks + 1,
             n_thr, max_objects]; field float64 [n_blocks + 1, 3]; field_cells uint32 [n_blocks + 1, 2].
  Limits     the accumulators, SUM_BINS int64 per table row and per source, and the weight table count into the scratch limit.

MATCH (Objects(match=True); `pairs`, `match` and `contingency` read it).  It needs neither `labels` nor `sums`; neither changes.
  For every block b and threshold t:
  Label maps lf = the label map of source b, lo = that of the observed map (source n_blocks), both at threshold t exactly as
             'labels' defines them: kept objects only (min_area applied), numbers 1 ... n_objects, complete beyond max_objects.
  Overlap    I = (lf > 0) & (lo > 0).
  Piece      a maximal set of cells of I connected through `connectivity`.  Every piece lies in exactly one forecast object and
             one observed object.
  Numbering  the pieces are numbered 1 ... n in ascending order of their first cell (the smallest flat index); no area filter.
  Piece row  WORDS uint32: first, area, sum of ix, sum of iy, x0, x1, y0, y1 (an object row's first eight words), then forecast
             (the piece's number in lf) and observed (its number in lo).  The no-overflow clause holds as for the objects.
  Outputs    n_pieces uint32 [n_blocks, n_thr]: the true count, also beyond max_pieces; pieces uint32 [n_blocks, n_thr,
             max_pieces, WORDS], rows at or beyond n_pieces zero; covered uint32 [n_blocks, n_thr, 2, max_objects]: side 0, entry
             k - 1: the cells of forecast object k of block b that lie in I; side 1, entry k - 1: the cells of observed object k
             that lie in I against block b; entries at or beyond min(n_objects, max_objects) of that side zero.  `covered` is
             counted from the cells: complete whatever max_pieces is.
  Invariants nothing overflowing: sum of the pieces' areas == sum of covered[0] == sum of covered[1] == the cells of I;
             covered[0][k - 1] <= the area of object k.
  The rule   `pieces_of_map`, built on `cells_of_map`.  Every number is a count, an integer sum, an integer extreme or a
             comparison: the device result equals it exactly.
  Limits     the piece scratch, n_blocks * n_thr * (2 * n_y * n_x + n_y) * 4 bytes, counts into the scratch limit.

TRACK (Objects(track=True, max_shift=S | shifts=...); `links`, `tracks` and `motion` read it).  The blocks of the call are scan
times: block p is followed into block p + 1.  It needs neither `labels`, `sums` nor `match`; none of them changes.
  Pairs      a call has B = n_blocks >= 2 blocks and P = B - 1 pairs; pair p is (earlier = block p, later = block p + 1).
  Per pair and threshold t: le, ll = the label maps of the two blocks exactly as 'labels' defines them (kept objects only,
             min_area applied, complete beyond max_objects); Ke = le > 0, Kl = ll > 0.
  Correlation for |dy|, |dx| <= S = max_shift (0 ... TRACK_MAX_SHIFT = 32): C[dy + S, dx + S] = #{(y, x): Ke[y, x] and
             Kl[y + dy, x + dx]}, both cells inside the grid; uint32 (a count is below 2^20).  S may exceed the grid's sides:
             such offsets count 0.  `correlation_of_pair`.
  Shift      the (dy, dx) with the largest C; ties go to the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx.
             An all-zero table gives (0, 0).  `shift_of`.
  Given      instead of max_shift the caller may hand `shifts`: int32, broadcastable to [P, n_thr, 2] (dy, dx), |dy|, |dx| <=
             TRACK_MAX_GIVEN = 1023 (a model-wind guess); no correlation is then computed or delivered.  The shape is checked at
             the call, where P is known.
  Overlap    le'[y, x] = le[y - dy, x - dx] inside the grid, 0 outside (`shift_labels`).  The pieces, n_pieces and covered of the
             pair are pieces_of_map(le', ll, connectivity, max_track_pieces, max_objects), unchanged, in the later block's frame:
             the word `forecast` is the object's number in the earlier block, `observed` its number in the later block;
             covered[0] counts cells of the earlier objects, covered[1] cells of the later ones.  The invariants of MATCH hold.
  Outputs    res['track'] = {'correlation': uint32 [P, n_thr, 2S + 1, 2S + 1] (None with given shifts), 'shift': int32 [P, n_thr,
             2], 'n_pieces': uint32 [P, n_thr] (the true count), 'pieces': uint32 [P, n_thr, max_track_pieces, WORDS] (rows at or
             beyond n_pieces zero), 'covered': uint32 [P, n_thr, 2, max_objects]}.  `track_of_maps`.
  Limits     the track scratch, behind everything else on an 8-byte boundary: the packed masks, n_blocks * n_thr * n_y *
             ceil(n_x / 64) * 8 bytes, and P * n_thr piece maps of (2 * n_y * n_x + n_y) * 4 bytes, counts into the scratch limit.
  Not built  tracking across calls; tracks of layered composites; per-object (local) shifts; a process group."""
import numpy as np

from . import neighbourhood as NB

WORDS = 10
MAX_OBJECTS = 65535
MAX_SCRATCH_BYTES = 1 << 30
TRACK_MAX_SHIFT, TRACK_MAX_GIVEN = 32, 1023                # CPOL_TRACK_MAX_SHIFT, CPOL_TRACK_MAX_GIVEN
MAX_TABLE = 1024                                          # breakpoints of a weight table: the composite's MAX_TABLE
SUM_BINS = 16 + 32 + 32                                   # int64 bins of one accumulator row (cpol_obj.h): volume, moment_x, moment_y
FIRST, AREA, SUM_X, SUM_Y, X0, X1, Y0, Y1, PEAK_CELL, PEAK_BITS = range(WORDS)
FORECAST, OBSERVED = PEAK_CELL, PEAK_BITS                 # a piece row: the two peak words give way to the two numbers

_U32, _I64 = np.uint32, np.int64


class Objects(object):
    """What a call with object cells finds: the cells of the binary maps of `fractions` (a neighbourhood.Fractions) under
    `connectivity` 4 or 8, those below `min_area` cells dropped, up to `max_objects` (1 ... 65535) table rows per source and
    threshold, with the label maps when `labels` and the exact sums when `sums`, under `weight` = (table_v, table_f) or None
    (w = m), and with the overlap pieces of every block against the observed map when `match`, up to `max_pieces` (1 ... 65535,
    default max_objects) rows per block and threshold; and with the track of every block's objects into the next block when
    `track` (TRACK above): exactly one of `max_shift` (0 ... 32: the displacement is found) and `shifts` (int32, broadcastable to
    [n_blocks - 1, n_thr, 2]: it is given), up to `max_track_pieces` (1 ... 65535, default max_objects) rows per pair and
    threshold.  ValueError for what the library refuses.  The Fractions is `fractions`; the properties the scored entry points
    read of a spec are its own."""

    def __init__(self, fractions, connectivity=4, min_area=1, max_objects=1024, labels=True, sums=False, weight=None, match=False,
                 max_pieces=None, track=False, max_shift=None, shifts=None, max_track_pieces=None):
        if not isinstance(fractions, NB.Fractions):
            raise ValueError('fractions: a cosmo_pol_amd.neighbourhood.Fractions, got %r' % (fractions,))
        for name, v in (('connectivity', connectivity), ('min_area', min_area), ('max_objects', max_objects)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError('%s: an integer, got %r' % (name, v))
        if connectivity not in (4, 8):
            raise ValueError('connectivity must be 4 or 8, got %r' % (connectivity,))
        if min_area < 1:
            raise ValueError('min_area must be at least 1, got %r' % (min_area,))
        if not 1 <= max_objects <= MAX_OBJECTS:
            raise ValueError('max_objects must lie in 1 ... %d, got %r' % (MAX_OBJECTS, max_objects))
        self.fractions = fractions
        self.connectivity, self.min_area, self.max_objects, self.labels = int(connectivity), int(min_area), int(max_objects), bool(labels)
        self.sums, self.weight = bool(sums), None
        if weight is not None:
            if not self.sums:
                raise ValueError('weight: a weight table belongs to sums=True')
            self.weight = check_weight(weight)
        self.match, self.max_pieces = bool(match), None
        if max_pieces is not None and not self.match:
            raise ValueError('max_pieces: belongs to match=True')
        if self.match:
            max_pieces = self.max_objects if max_pieces is None else max_pieces
            if isinstance(max_pieces, (bool, np.bool_)) or not isinstance(max_pieces, (int, np.integer)):
                raise ValueError('max_pieces: an integer, got %r' % (max_pieces,))
            if not 1 <= max_pieces <= MAX_OBJECTS:
                raise ValueError('max_pieces must lie in 1 ... %d, got %r' % (MAX_OBJECTS, max_pieces))
            self.max_pieces = int(max_pieces)
        self.track, self.max_shift, self.shifts, self.max_track_pieces = bool(track), None, None, None
        if not self.track:
            for name, v in (('max_shift', max_shift), ('shifts', shifts), ('max_track_pieces', max_track_pieces)):
                if v is not None:
                    raise ValueError('%s: belongs to track=True' % name)
        else:
            if (max_shift is None) == (shifts is None):
                raise ValueError('track=True needs exactly one of max_shift and shifts')
            if max_shift is not None:
                if isinstance(max_shift, (bool, np.bool_)) or not isinstance(max_shift, (int, np.integer)):
                    raise ValueError('max_shift: an integer, got %r' % (max_shift,))
                if not 0 <= max_shift <= TRACK_MAX_SHIFT:
                    raise ValueError('max_shift must lie in 0 ... %d, got %r' % (TRACK_MAX_SHIFT, max_shift))
                self.max_shift = int(max_shift)
            else:
                self.shifts = check_shifts(shifts)
            max_track_pieces = self.max_objects if max_track_pieces is None else max_track_pieces
            if isinstance(max_track_pieces, (bool, np.bool_)) or not isinstance(max_track_pieces, (int, np.integer)):
                raise ValueError('max_track_pieces: an integer, got %r' % (max_track_pieces,))
            if not 1 <= max_track_pieces <= MAX_OBJECTS:
                raise ValueError('max_track_pieces must lie in 1 ... %d, got %r' % (MAX_OBJECTS, max_track_pieces))
            self.max_track_pieces = int(max_track_pieces)

    composite = property(lambda self: self.fractions.composite)
    thresholds = property(lambda self: self.fractions.thresholds)
    n_x = property(lambda self: self.fractions.n_x)
    n_y = property(lambda self: self.fractions.n_y)

    @property
    def key(self):
        key = (self.fractions.key, self.connectivity, self.min_area, self.max_objects, self.labels)
        if self.sums:
            key += (True, None if self.weight is None else (self.weight[0].tobytes(), self.weight[1].tobytes()))
        if self.match:
            key += ('match', self.max_pieces)
        if self.track:
            key += ('track', self.max_shift, None if self.shifts is None else (self.shifts.shape, self.shifts.tobytes()), self.max_track_pieces)
        return key

    def __eq__(self, other):
        return isinstance(other, Objects) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        tail = ''
        if self.sums:
            tail = ', sums=True' + ('' if self.weight is None else ', weight=<%d breakpoints>' % len(self.weight[0]))
        if self.match:
            tail += ', match=True, max_pieces=%d' % self.max_pieces
        if self.track:
            tail += ', track=True, %s, max_track_pieces=%d' % (
                'max_shift=%d' % self.max_shift if self.shifts is None else 'shifts=<%s>' % 'x'.join(map(str, self.shifts.shape)), self.max_track_pieces)
        return 'Objects(%r, connectivity=%d, min_area=%d, max_objects=%d, labels=%r%s)' % (
            self.fractions, self.connectivity, self.min_area, self.max_objects, self.labels, tail)


def check_weight(weight):
    """(table_v float32, table_f float64) of a weight table as the library takes it; ValueError for what it refuses."""
    try:
        tv, tf = weight
        with np.errstate(over='ignore'):
            tv, tf = np.ascontiguousarray(tv, dtype=np.float32), np.ascontiguousarray(tf, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('weight: (table_v, table_f), got %r' % (weight,))
    if tv.ndim != 1 or tv.shape != tf.shape or not 2 <= tv.size <= MAX_TABLE:
        raise ValueError('weight: two arrays of 2 ... %d breakpoints' % MAX_TABLE)
    if not (np.isfinite(tv).all() and np.isfinite(tf).all()):
        raise ValueError('weight: a breakpoint or a value is NaN or infinite')
    if np.any(tv[1:] <= tv[:-1]):
        raise ValueError('weight: the breakpoints are not strictly ascending')
    if np.any(tf[1:] < tf[:-1]):
        raise ValueError('weight: the values decrease')
    return tv, tf


def check_shifts(shifts):
    """int32 [..., 2] of given shifts as the library takes them (at most three axes, the last one (dy, dx)); ValueError else.
    That they broadcast to [n_blocks - 1, n_thr, 2] is checked at the call (`shifts_of_call`)."""
    try:
        a = np.asarray(shifts)
    except (TypeError, ValueError):
        raise ValueError('shifts: an integer array [..., 2], got %r' % (shifts,))
    if a.dtype.kind not in 'iu' or a.ndim < 1 or a.ndim > 3 or a.shape[-1] != 2:
        raise ValueError('shifts: integers (dy, dx), broadcastable to [n_blocks - 1, n_thr, 2], got %s %r' % (a.dtype, a.shape))
    if a.size and (a.min() < -TRACK_MAX_GIVEN or a.max() > TRACK_MAX_GIVEN):
        raise ValueError('shifts: |dy| and |dx| at most %d' % TRACK_MAX_GIVEN)
    return np.ascontiguousarray(a, dtype=np.int32)


def shifts_of_call(spec, n_blocks):
    """int32 [n_blocks - 1, n_thr, 2], contiguous: the given shifts of a call of `n_blocks` blocks; ValueError when the spec's do not
    broadcast to it, and for a call of one block."""
    if n_blocks < 2:
        raise ValueError('track: the call yields %d block; tracking needs at least two (rays_per_block, or a series of times)' % n_blocks)
    shape = (n_blocks - 1, len(spec.thresholds), 2)
    try:
        return np.ascontiguousarray(np.broadcast_to(spec.shifts, shape), dtype=np.int32)
    except ValueError:
        raise ValueError('shifts: %r does not broadcast to [n_blocks - 1, n_thr, 2] = %r' % (spec.shifts.shape, shape))


def scratch_bytes(spec, blocks):
    """The bytes of the scratch of `blocks` blocks and the observation (cpol_obj.h): the labelling's and, with the exact sums,
    behind it on an 8-byte boundary the accumulators and the weight table, and with the match behind those on an 8-byte boundary
    the piece scratch of `blocks` blocks, and with the track behind those on an 8-byte boundary the packed masks of `blocks`
    blocks and the piece scratch of `blocks` - 1 pairs."""
    maps = (int(blocks) + 1) * len(spec.thresholds)
    n = maps * (2 * spec.n_y * spec.n_x + spec.n_y) * 4
    if getattr(spec, 'sums', False):
        nw = 0 if spec.weight is None else len(spec.weight[0])
        n = (n + 7) // 8 * 8 + (maps * spec.max_objects + int(blocks) + 1) * SUM_BINS * 8 + nw * 8 + (nw * 4 + 7) // 8 * 8
    if getattr(spec, 'match', False):
        n = (n + 7) // 8 * 8 + int(blocks) * len(spec.thresholds) * (2 * spec.n_y * spec.n_x + spec.n_y) * 4
    if getattr(spec, 'track', False):
        n = (n + 7) // 8 * 8 + int(blocks) * len(spec.thresholds) * spec.n_y * ((spec.n_x + 63) // 64) * 8
        n += (int(blocks) - 1) * len(spec.thresholds) * (2 * spec.n_y * spec.n_x + spec.n_y) * 4
    return n


# ---------------------------------------------------------------------------------------------------- the exact sums
def split(values):
    """(negative bool, E int64, M int64, finite bool) of float32 values: a finite value is +-M * 2 ** (E - 150) with E = max(e, 1)
    and M below 2 ** 24 (cpol_obj.h, obj_sum_split)."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(_U32)
    e = ((bits >> _U32(23)) & _U32(0xFF)).astype(_I64)
    m = (bits & _U32(0x007FFFFF)).astype(_I64)
    return (bits >> _U32(31)) != 0, np.maximum(e, 1), np.where(e > 0, m | 0x00800000, m), e != 0xFF


def round_scaled(total):
    """The float64 nearest to the Python integer `total` times 2 ** -150, ties to even, by hand: the top 53 bits, then half-to-even
    on the remainder; +0.0 for zero (cpol_obj.h, obj_sum_round).  |total| < 2 ** 1000."""
    total = int(total)
    if total == 0:
        return np.float64(0.0)
    mag = abs(total)
    p = mag.bit_length() - 1
    if p <= 52:
        mant = mag << (52 - p)
    else:
        r = p - 52
        mant, rem, half = mag >> r, mag & ((1 << r) - 1), 1 << (r - 1)
        if rem > half or (rem == half and mant & 1):
            mant += 1                                     # (2 ** 53: the sum below carries it into the exponent)
    bits = ((p - 150 + 1023) << 52) + (mant - (1 << 52)) | ((1 << 63) if total < 0 else 0)
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def exact_sum(values, mult=None):
    """float64: the sum of the finite float32 `values` (times the integers `mult`, 0 ... 1023, when given), formed exactly and
    rounded once, round-to-nearest-even: math.fsum of the summands in any order.  Integer arithmetic alone."""
    neg, E, M, finite = split(np.asarray(values, dtype=np.float32).reshape(-1))
    if not finite.all():
        raise ValueError('exact_sum: the values must be finite')
    if mult is not None:
        mult = np.asarray(mult).reshape(-1)
        if mult.shape != M.shape or mult.dtype.kind not in 'iu' or (mult.size and (mult.min() < 0 or mult.max() > 1023)):
            raise ValueError('exact_sum: mult: one integer in 0 ... 1023 per value')
        M = M * mult.astype(_I64)
    total = 0
    for n, e, m in zip(neg.tolist(), E.tolist(), M.tolist()):
        total += -(m << e) if n else m << e
    return round_scaled(total)


def weight_of(values, weight=None):
    """float32: the summand w of float32 plane values under `weight` = (table_v, table_f) or None (w = m): float32(f(m)),
    statement by statement what composite.column_of does per layer.  NaN stays NaN (such a cell is never summed)."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    if weight is None:
        return v
    tv, tf = weight
    n = len(tv)
    tv64 = tv.astype(np.float64)
    have = v == v
    with np.errstate(invalid='ignore', over='ignore'):
        i = np.searchsorted(tv, np.where(have, v, tv[0]), side='right') - 1
        ii = np.clip(i, 0, n - 2)
        t = (v.astype(np.float64) - tv64[ii]) / (tv64[ii + 1] - tv64[ii])
        d = tf[ii + 1] - tf[ii]
        p = t * d
        f = tf[ii] + p
        f = np.where(i < 0, 0.0, np.where(i >= n - 1, tf[n - 1], f))
        return np.where(have, f, np.nan).astype(np.float32)


def zr_table(a=200.0, b=1.6, db_min=0.0, db_cap=60.0, step_db=0.25):
    """The weight table of the rain rate under Z = a * R ** b (Marshall and Palmer 1948: a = 200, b = 1.6), Z in mm^6 m^-3, R in
    mm h^-1: (float32 Z breakpoints every `step_db` from `db_min` to `db_cap` dBZ, float64 R = (Z / a) ** (1 / b) at the ROUNDED
    breakpoints), in the manner of composite.vil_table.  Below db_min a cell adds nothing; at and above db_cap the rate stays
    that of db_cap (the cap against hail).  The values never decrease."""
    a, b, db_min, db_cap, step_db = float(a), float(b), float(db_min), float(db_cap), float(step_db)
    if not (a > 0.0 and b > 0.0 and step_db > 0.0 and db_cap > db_min):
        raise ValueError('zr_table: a > 0, b > 0, db_min < db_cap and step_db > 0')
    n = int(round((db_cap - db_min) / step_db)) + 1
    if not 2 <= n <= MAX_TABLE:
        raise ValueError('zr_table: %d breakpoints; 2 ... %d' % (n, MAX_TABLE))
    db = db_min + step_db * np.arange(n, dtype=np.float64)
    db[-1] = db_cap
    tv = (10.0 ** (db / 10.0)).astype(np.float32)
    return tv, np.maximum.accumulate(np.power(tv.astype(np.float64) / a, 1.0 / b))


def group_sums(w, ix, iy, group, n_groups):
    """(float64 [n_groups, 3], uint32 [n_groups]): volume, moment_x and moment_y of the cells with weights `w` (float32, no NaN) at
    (ix, iy) per group 0 ... n_groups - 1, and the cells skipped (w infinite).  The accumulator rows of cpol_obj.h in int64 -- no
    bin can wrap: below 2 ** 20 cells, the sum of ix below 2 ** 30 -- then every row folded into ONE Python integer and rounded."""
    neg, E, M, finite = split(w)
    group = np.asarray(group, dtype=_I64)
    skipped = np.bincount(group[~finite], minlength=n_groups).astype(_U32)
    g, E, ix, iy = group[finite], E[finite], np.asarray(ix, dtype=_I64)[finite], np.asarray(iy, dtype=_I64)[finite]
    M = np.where(neg[finite], -M[finite], M[finite])
    acc = np.zeros((n_groups, SUM_BINS), dtype=_I64)
    np.add.at(acc, (g, E >> 4), M << (E & 15))
    np.add.at(acc, (g, 16 + (E >> 3)), (M * ix) << (E & 7))
    np.add.at(acc, (g, 48 + (E >> 3)), (M * iy) << (E & 7))
    out = np.zeros((n_groups, 3), dtype=np.float64)
    for k, row in enumerate(acc.tolist()):
        out[k, 0] = round_scaled(sum(v << (16 * b) for b, v in enumerate(row[:16]) if v))
        out[k, 1] = round_scaled(sum(v << (8 * b) for b, v in enumerate(row[16:48]) if v))
        out[k, 2] = round_scaled(sum(v << (8 * b) for b, v in enumerate(row[48:]) if v))
    return out, skipped


def sums_of_map(lab, n, w, max_objects):
    """The exact sums of ONE label map: (float64 [max_objects, 3], uint32 [max_objects]) of the objects 1 ... min(n, max_objects);
    w: the weights of the map's cells, float32."""
    volume, skipped = np.zeros((max_objects, 3), dtype=np.float64), np.zeros(max_objects, dtype=_U32)
    rows = min(int(n), max_objects)
    if rows:
        flat = np.flatnonzero((lab > 0) & (lab <= rows))
        n_x = lab.shape[1]
        volume[:rows], skipped[:rows] = group_sums(w.reshape(-1)[flat], flat % n_x, flat // n_x, lab.reshape(-1)[flat].astype(_I64) - 1, rows)
    return volume, skipped


def sums_of_field(values, w, dom):
    """(float64 [3], uint32 [2]): the sums over every cell of the field with dom && m == m; the cells summed, the cells skipped."""
    flat = np.flatnonzero(dom & (values == values))
    n_x = values.shape[1]
    s, k = group_sums(w.reshape(-1)[flat], flat % n_x, flat // n_x, np.zeros(flat.size, dtype=_I64), 1)
    return s[0], np.array([flat.size - int(k[0]), k[0]], dtype=_U32)


def _runs(binary):
    """The row runs of a bool map in raster order: (row, first x, one past the last x), int64 each."""
    n_y, n_x = binary.shape
    pad = np.zeros((n_y, n_x + 2), dtype=np.int8)
    pad[:, 1:-1] = binary
    d = np.diff(pad, axis=1).reshape(-1)                  # [n_y * (n_x + 1)]: +1 where a run begins, -1 one past where it ends
    begin, end = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return begin // (n_x + 1), begin % (n_x + 1), end % (n_x + 1)


def label(binary, connectivity=4):
    """(labels int32 [n_y, n_x], n): the objects of the bool map `binary` under `connectivity` 4 or 8, numbered 1 ... n in
    ascending order of their first cells, 0 for background -- scipy.ndimage.label's result, without SciPy.  A union-find over
    the row runs: the pairs of touching runs of adjacent rows from two binary searches, then hooking to the smaller label and
    pointer jumping until nothing changes."""
    binary = np.asarray(binary)
    if binary.ndim != 2 or binary.dtype != np.bool_:
        raise ValueError('binary: a 2-D bool array, got %s %r' % (binary.dtype, binary.shape))
    if connectivity not in (4, 8):
        raise ValueError('connectivity must be 4 or 8, got %r' % (connectivity,))
    n_y, n_x = binary.shape
    out = np.zeros((n_y, n_x), dtype=np.int32)
    row, x0, x1 = _runs(binary)
    n_runs = row.size
    if n_runs == 0:
        return out, 0
    reach = 1 if connectivity == 8 else 0
    W = n_x + 2                                           # (a row's keys end two short of the next row's: no run of another row matches)
    key_begin, key_end = row * W + x0, row * W + x1
    # the runs of the row above with  begin < x1 + reach  and  end > x0 - reach
    lo = np.searchsorted(key_end, (row - 1) * W + x0 - reach, side='right')
    hi = np.searchsorted(key_begin, (row - 1) * W + x1 + reach, side='left')
    n_pairs = np.maximum(hi - lo, 0)
    n_pairs[row == 0] = 0
    a = np.repeat(np.arange(n_runs), n_pairs)
    b = np.repeat(lo - (np.cumsum(n_pairs) - n_pairs), n_pairs) + np.arange(a.size)
    lab = np.arange(n_runs)
    while a.size:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        for target in (lab[a], lab[b], a, b):
            np.minimum.at(new, target, m)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            break
        lab = new
    # (a label is the smallest run of its object, and the runs lie in raster order: ascending labels are ascending first cells)
    roots, number = np.unique(lab, return_inverse=True)
    out[binary] = np.repeat(number.reshape(-1) + 1, x1 - x0).astype(np.int32)
    return out, int(roots.size)


def float_order(values):
    """uint32: the place of float32 values in the total order in which -0.0 lies before +0.0 (cpol_obj.h, obj_order)."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(_U32)
    return np.where(bits & _U32(0x80000000), ~bits, bits | _U32(0x80000000))


def _table(lab, n, values, max_objects):
    """uint32 [max_objects, WORDS]: the rows of the objects 1 ... min(n, max_objects) of the label map `lab`."""
    table = np.zeros((max_objects, WORDS), dtype=_U32)
    rows = min(n, max_objects)
    if rows == 0:
        return table
    n_x = lab.shape[1]
    flat = np.flatnonzero((lab > 0) & (lab <= rows))      # ascending flat index
    k = lab.reshape(-1)[flat].astype(_I64) - 1
    iy, ix = flat // n_x, flat % n_x

    def low(v):
        o = np.full(rows, np.iinfo(_I64).max, dtype=_I64)
        np.minimum.at(o, k, v)
        return o

    def high(v):
        o = np.full(rows, -1, dtype=_I64)
        np.maximum.at(o, k, v)
        return o
    table[:rows, FIRST] = low(flat)
    table[:rows, AREA] = np.bincount(k, minlength=rows)
    table[:rows, SUM_X] = np.bincount(k, weights=ix, minlength=rows).astype(_I64)     # (< 2^30: exact in float64)
    table[:rows, SUM_Y] = np.bincount(k, weights=iy, minlength=rows).astype(_I64)
    table[:rows, X0], table[:rows, X1], table[:rows, Y0], table[:rows, Y1] = low(ix), high(ix), low(iy), high(iy)
    order = float_order(values.reshape(-1)[flat]).astype(_I64)
    best = high(order)
    at_peak = order == best[k]
    peak_cell = low(np.where(at_peak, flat, np.iinfo(_I64).max))
    table[:rows, PEAK_CELL] = peak_cell
    table[:rows, PEAK_BITS] = np.ascontiguousarray(values, dtype=np.float32).view(_U32).reshape(-1)[peak_cell]
    return table


def cells_of_map(binary, values, connectivity, min_area, max_objects):
    """The rule for ONE binary map: (n uint32, table uint32 [max_objects, WORDS], labels int32 [n_y, n_x])."""
    lab, n = label(binary, connectivity)
    if min_area > 1 and n:
        area = np.bincount(lab.reshape(-1), minlength=n + 1)
        keep = area >= min_area
        keep[0] = False
        number = np.where(keep, np.cumsum(keep), 0).astype(np.int32)      # (the kept keep their order)
        lab, n = number[lab], int(keep.sum())
    return _U32(n), _table(lab, n, values, max_objects), lab


def pieces_of_map(lf, lo, connectivity, max_pieces, max_objects):
    """The rule of the match for ONE pair of label maps (int32 [n_y, n_x], as `cells_of_map` returns them): (n_pieces uint32,
    pieces uint32 [max_pieces, WORDS], covered uint32 [2, max_objects])."""
    both = (lf > 0) & (lo > 0)
    n, pieces, _ = cells_of_map(both, np.zeros(both.shape, dtype=np.float32), connectivity, 1, max_pieces)
    rows = min(int(n), max_pieces)
    pieces[:, PEAK_CELL:] = 0                             # (no peak: the two words are the numbers)
    pieces[:rows, FORECAST] = lf.reshape(-1)[pieces[:rows, FIRST]]
    pieces[:rows, OBSERVED] = lo.reshape(-1)[pieces[:rows, FIRST]]
    covered = np.zeros((2, max_objects), dtype=_U32)
    for side, lab in enumerate((lf, lo)):
        k = lab[both].astype(_I64)
        covered[side] = np.bincount(k[k <= max_objects] - 1, minlength=max_objects)
    return n, pieces, covered


# ---------------------------------------------------------------------------------------------------- the track
def correlation_of_pair(le, ll, S):
    """uint32 [2S + 1, 2S + 1]: C[dy + S, dx + S] = the cells (y, x) with le[y, x] > 0 and ll[y + dy, x + dx] > 0, both inside the
    grid, for |dy|, |dx| <= S (TRACK, Correlation).  le, ll: label maps (or bool maps) of one shape."""
    ke, kl = np.asarray(le) > 0, np.asarray(ll) > 0
    S = int(S)
    if ke.ndim != 2 or ke.shape != kl.shape or S < 0:
        raise ValueError('correlation_of_pair: two maps of one shape and S >= 0')
    n_y, n_x = ke.shape
    C = np.zeros((2 * S + 1, 2 * S + 1), dtype=_U32)
    for dy in range(-min(S, n_y - 1), min(S, n_y - 1) + 1):
        e_rows, l_rows = ke[max(0, -dy):n_y - max(0, dy)], kl[max(0, dy):n_y - max(0, -dy)]
        for dx in range(-min(S, n_x - 1), min(S, n_x - 1) + 1):
            C[dy + S, dx + S] = np.count_nonzero(e_rows[:, max(0, -dx):n_x - max(0, dx)] & l_rows[:, max(0, dx):n_x - max(0, -dx)])
    return C


def shift_of(C):
    """(dy, dx): the offset with the largest count of a correlation table [2S + 1, 2S + 1]; ties go to the smallest dy^2 + dx^2,
    then the smallest dy, then the smallest dx (TRACK, Shift).  An all-zero table gives (0, 0)."""
    C = np.asarray(C)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or C.shape[0] % 2 != 1:
        raise ValueError('shift_of: a table [2S + 1, 2S + 1], got %r' % (C.shape,))
    S = C.shape[0] // 2
    dy, dx = [q.reshape(-1) for q in np.meshgrid(np.arange(-S, S + 1), np.arange(-S, S + 1), indexing='ij')]
    best = np.lexsort((dx, dy, dy * dy + dx * dx, -C.reshape(-1).astype(_I64)))[0]      # (the last key is the first criterion)
    return int(dy[best]), int(dx[best])


def shift_labels(le, dy, dx):
    """le'[y, x] = le[y - dy, x - dx] inside the grid, 0 outside (TRACK, Overlap): the map moved by (dy, dx)."""
    le = np.asarray(le)
    n_y, n_x = le.shape
    out = np.zeros_like(le)
    dy, dx = int(dy), int(dx)
    if abs(dy) < n_y and abs(dx) < n_x:
        out[max(0, dy):n_y - max(0, -dy), max(0, dx):n_x - max(0, -dx)] = le[max(0, -dy):n_y - max(0, dy), max(0, -dx):n_x - max(0, dx)]
    return out


def track_of_labels(spec, labels):
    """The track of the label maps int32 [n_blocks, n_thr, n_y, n_x] of a call's blocks: (correlation or None, shift, n_pieces,
    pieces, covered) as TRACK's Outputs describe them."""
    n_blocks, n_thr = labels.shape[:2]
    P = n_blocks - 1
    given = None if spec.shifts is None else shifts_of_call(spec, n_blocks)
    if P < 1:
        raise ValueError('track: %d block; tracking needs at least two' % n_blocks)
    S = spec.max_shift
    corr = None if given is not None else np.zeros((P, n_thr, 2 * S + 1, 2 * S + 1), dtype=_U32)
    shift = np.zeros((P, n_thr, 2), dtype=np.int32)
    n = np.zeros((P, n_thr), dtype=_U32)
    pieces = np.zeros((P, n_thr, spec.max_track_pieces, WORDS), dtype=_U32)
    covered = np.zeros((P, n_thr, 2, spec.max_objects), dtype=_U32)
    for p in range(P):
        for t in range(n_thr):
            le, ll = labels[p, t], labels[p + 1, t]
            if given is None:
                corr[p, t] = correlation_of_pair(le, ll, S)
                shift[p, t] = shift_of(corr[p, t])
            else:
                shift[p, t] = given[p, t]
            n[p, t], pieces[p, t], covered[p, t] = pieces_of_map(shift_labels(le, *shift[p, t]), ll, spec.connectivity,
                                                                 spec.max_track_pieces, spec.max_objects)
    return corr, shift, n, pieces, covered


def track_result(arrays):
    """The five arrays of the track named: res['track']."""
    return dict(zip(('correlation', 'shift', 'n_pieces', 'pieces', 'covered'), arrays))


def track_of_maps(spec, plane_maps, domain=None):
    """The rule of the track in NumPy: res['track'] of the scored plane's blocks float32 [n_blocks, n_y, n_x] under `spec` (an
    Objects with track=True) -- exactly what the device returns.  The observed map plays no part."""
    if not getattr(spec, 'track', False):
        raise ValueError('track_of_maps: the spec has no track (Objects(track=True))')
    m = np.asarray(plane_maps)
    F = binary_maps(spec.fractions, m, np.zeros((spec.n_y, spec.n_x), dtype=np.float32), domain)[0]
    labels = np.zeros(F.shape, dtype=np.int32)
    for b in range(F.shape[0]):
        for t in range(F.shape[1]):
            labels[b, t] = cells_of_map(F[b, t], np.zeros(F.shape[2:], dtype=np.float32), spec.connectivity, spec.min_area, 1)[2]
    return track_result(track_of_labels(spec, labels))


def result(spec, n_objects, table, labels=None, sums=None, match=None, track=None):
    """The output arrays named.  n_objects [n_blocks + 1, n_thr], table [n_blocks + 1, n_thr, max_objects, WORDS], labels
    [n_blocks + 1, n_thr, n_y, n_x] or None -> {'n_objects': uint32 [n_blocks, n_thr], 'first' | 'area' | 'sum_x' | 'sum_y' |
    'peak_cell': uint32 [n_blocks, n_thr, max_objects], 'bbox': uint32 [..., 4] (x0, x1, y0, y1), 'peak': float32 [...],
    'labels': int32 [n_blocks, n_thr, n_y, n_x] (when given), 'observed': the same of the observed map without the leading
    axis, 'connectivity', 'min_area', 'thresholds'}.  sums: None or the four arrays of the exact sums (volume [n_blocks + 1,
    n_thr, max_objects, 3], skipped, field [n_blocks + 1, 3], field_cells [n_blocks + 1, 2]): 'volume' | 'moment_x' | 'moment_y':
    float64 [n_blocks, n_thr, max_objects], 'skipped': uint32 likewise, 'field': {'volume', 'moment_x', 'moment_y': float64
    [n_blocks], 'cells', 'skipped': uint32 [n_blocks]}, the same under 'observed', and 'weight' (the spec's table or None) and
    'grid' (n_y, n_x) for `sal`.  match: None or the three arrays of the match (n_pieces [n_blocks, n_thr], pieces [n_blocks,
    n_thr, max_pieces, WORDS], covered [n_blocks, n_thr, 2, max_objects]): 'pieces': {'n_pieces': uint32 [n_blocks, n_thr],
    'first' | 'area' | 'sum_x' | 'sum_y' | 'forecast' | 'observed': uint32 [n_blocks, n_thr, max_pieces], 'bbox': [..., 4]},
    'covered' and 'covered_observed': uint32 [n_blocks, n_thr, max_objects].  track: None or the five arrays of the track
    (correlation or None, shift, n_pieces, pieces, covered: TRACK, Outputs): 'track', under those names."""
    def named(n, tb, lb, sm=None):
        out = {'n_objects': n, 'first': tb[..., FIRST], 'area': tb[..., AREA], 'sum_x': tb[..., SUM_X], 'sum_y': tb[..., SUM_Y],
               'bbox': tb[..., X0:Y1 + 1], 'peak': tb[..., PEAK_BITS].view(np.float32),     # (views all: a pinned call fills them later)
               'peak_cell': tb[..., PEAK_CELL]}
        if lb is not None:
            out['labels'] = lb
        if sm is not None:
            vol, skipped, field, field_cells = sm
            out.update(volume=vol[..., 0], moment_x=vol[..., 1], moment_y=vol[..., 2], skipped=skipped,
                       field={'volume': field[..., 0], 'moment_x': field[..., 1], 'moment_y': field[..., 2],
                              'cells': field_cells[..., 0], 'skipped': field_cells[..., 1]})
        return out
    out = named(n_objects[:-1], table[:-1], None if labels is None else labels[:-1], None if sums is None else [q[:-1] for q in sums])
    out['observed'] = named(n_objects[-1], table[-1], None if labels is None else labels[-1], None if sums is None else [q[-1] for q in sums])
    out.update(connectivity=spec.connectivity, min_area=spec.min_area, thresholds=spec.thresholds)
    if sums is not None:
        out.update(weight=spec.weight, grid=(int(spec.n_y), int(spec.n_x)))
    if match is not None:
        n_pieces, pc, covered = match
        out['pieces'] = {'n_pieces': n_pieces, 'first': pc[..., FIRST], 'area': pc[..., AREA], 'sum_x': pc[..., SUM_X],
                         'sum_y': pc[..., SUM_Y], 'bbox': pc[..., X0:Y1 + 1], 'forecast': pc[..., FORECAST], 'observed': pc[..., OBSERVED]}
        out['covered'], out['covered_observed'] = covered[..., 0, :], covered[..., 1, :]
    if track is not None:
        out['track'] = track_result(track)
    return out


def binary_maps(fractions, plane_maps, observed, domain=None):
    """(F bool [n_blocks, n_thr, n_y, n_x], O bool [n_thr, n_y, n_x], m float32 [n_blocks, n_y, n_x], o): the binary maps of the
    rule, as neighbourhood.sums forms them."""
    m = np.asarray(plane_maps)
    if m.dtype != np.float32:
        raise ValueError('plane_maps must be float32, got %s' % m.dtype)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (fractions.n_y, fractions.n_x) or m.shape[0] < 1:
        raise ValueError('plane_maps: [n_blocks, %d, %d], got %r' % (fractions.n_y, fractions.n_x, m.shape))
    o, domain = NB.check_maps(fractions, observed, domain)
    dom = np.ones(o.shape, dtype=bool) if domain is None else domain != 0
    thr = fractions.thresholds[:, None, None]
    with np.errstate(invalid='ignore'):
        F = dom & (m == m)[:, None] & (m[:, None] >= thr)
        O = dom & (o == o) & (o[None] >= thr)
    return F, O, m, o


def cells(spec, plane_maps, observed, domain=None):
    """The rule in NumPy.  spec: an Objects (or any object with its attributes whose `fractions` has `thresholds`, `n_y` and
    `n_x`); plane_maps: float32 [n_blocks, n_y, n_x] (or [n_y, n_x]: one block), the scored plane as a composite's finish
    returns it; observed, domain: see neighbourhood.check_maps.  Returns what `result` describes -- exactly what the device
    returns ('labels' only with spec.labels; the keys of the exact sums only with spec.sums, those of the match only with
    spec.match, 'track' only with spec.track)."""
    F, O, m, o = binary_maps(spec.fractions, plane_maps, observed, domain)
    n_blocks, n_thr = F.shape[:2]
    with_sums = getattr(spec, 'sums', False)
    if with_sums:
        volume = np.zeros((n_blocks + 1, n_thr, spec.max_objects, 3), dtype=np.float64)
        skipped = np.zeros((n_blocks + 1, n_thr, spec.max_objects), dtype=_U32)
        field, field_cells = np.zeros((n_blocks + 1, 3), dtype=np.float64), np.zeros((n_blocks + 1, 2), dtype=_U32)
        dom = np.ones(o.shape, dtype=bool) if domain is None else NB.check_maps(spec.fractions, observed, domain)[1] != 0
    n = np.zeros((n_blocks + 1, n_thr), dtype=_U32)
    table = np.zeros((n_blocks + 1, n_thr, spec.max_objects, WORDS), dtype=_U32)
    labels = np.zeros((n_blocks + 1, n_thr) + o.shape, dtype=np.int32)
    for s in range(n_blocks + 1):
        if with_sums:
            values = m[s] if s < n_blocks else o
            w = weight_of(values, spec.weight)
            field[s], field_cells[s] = sums_of_field(values, w, dom)
        for t in range(n_thr):
            binary, values = (F[s, t], m[s]) if s < n_blocks else (O[t], o)
            n[s, t], table[s, t], labels[s, t] = cells_of_map(binary, values, spec.connectivity, spec.min_area, spec.max_objects)
            if with_sums:
                volume[s, t], skipped[s, t] = sums_of_map(labels[s, t], n[s, t], w, spec.max_objects)
    match = None
    if getattr(spec, 'match', False):
        match = (np.zeros((n_blocks, n_thr), dtype=_U32), np.zeros((n_blocks, n_thr, spec.max_pieces, WORDS), dtype=_U32),
                 np.zeros((n_blocks, n_thr, 2, spec.max_objects), dtype=_U32))
        for b in range(n_blocks):
            for t in range(n_thr):
                match[0][b, t], match[1][b, t], match[2][b, t] = pieces_of_map(labels[b, t], labels[n_blocks, t], spec.connectivity,
                                                                                spec.max_pieces, spec.max_objects)
    track = track_of_labels(spec, labels[:-1]) if getattr(spec, 'track', False) else None
    return result(spec, n, table, labels if spec.labels else None, (volume, skipped, field, field_cells) if with_sums else None, match, track)


def centroids(res):
    """float64 [..., max_objects, 2] (x, y): the centroids of the objects in GRID coordinates, sum / area plus the half cell (cell
    ix covers [ix, ix + 1)); NaN in the rows without an object.  `res`: what `result` returns, or its 'observed'."""
    area = res['area'].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        c = np.stack([res['sum_x'] / area + 0.5, res['sum_y'] / area + 0.5], axis=-1)
    return np.where((area > 0)[..., None], c, np.nan)


def weighted_centroids(res):
    """float64 [..., max_objects, 2] (x, y): the centroids of the objects weighted with w, moment / volume plus the half cell, in
    GRID coordinates; NaN where the volume is 0 or there is no object.  `res`: a result with the exact sums, or its 'observed'."""
    vol = res['volume']
    with np.errstate(invalid='ignore', divide='ignore'):
        c = np.stack([res['moment_x'] / vol + 0.5, res['moment_y'] / vol + 0.5], axis=-1)
    return np.where(((res['area'] > 0) & (vol != 0))[..., None], c, np.nan)


def _sal_side(side, t, n_max, weight):
    """Of one side and threshold index t: the field mean D, the field centre (x, y), the summed object volume R, the
    volume-weighted distance r of the object centroids to the field centre, the scaled volume V; leading axes kept."""
    fld = side['field']
    fv = fld['volume']
    with np.errstate(invalid='ignore', divide='ignore'):
        D = np.where(fld['cells'] > 0, fv / fld['cells'], np.nan)
        fx, fy = np.where(fv != 0, fld['moment_x'] / fv, np.nan), np.where(fv != 0, fld['moment_y'] / fv, np.nan)
        vol = side['volume'][..., t, :]
        have = side['area'][..., t, :] > 0
        cx = np.where(have, side['moment_x'][..., t, :] / vol, 0.0)
        cy = np.where(have, side['moment_y'][..., t, :] / vol, 0.0)
        dx, dy = cx - fx[..., None], cy - fy[..., None]
        R = np.where(have, vol, 0.0).sum(axis=-1)
        r = np.where(have, vol * np.sqrt(dx * dx + dy * dy), 0.0).sum(axis=-1) / R
        peak = weight_of(side['peak'][..., t, :], weight).astype(np.float64)
        V = np.where(have, vol * (vol / peak), 0.0).sum(axis=-1) / R
    bad = (side['n_objects'][..., t] < 1) | (side['n_objects'][..., t] > n_max) | ~(R != 0)
    return D, fx, fy, np.where(bad, np.nan, r), np.where(bad, np.nan, V)


def sal(res, threshold=0, d=None):
    """SAL (Wernli, Paulat, Hagen and Frei 2008, "SAL -- a novel quality measure for the verification of quantitative precipitation
    forecasts", Mon. Wea. Rev. 136, 4470-4487) of every block against the observed map from a result with the exact sums, for the
    objects of threshold index `threshold`: {'S', 'A', 'L', 'L1', 'L2'}, float64 [n_blocks].
      A   = (D_f - D_o) / (0.5 * (D_f + D_o)),  D = the field volume over the field's summed cells;
      L1  = |x_f - x_o| / d,  x = the field's centre of mass (moment / volume), d the largest distance in the domain: by default
            the grid's diagonal in cells;
      L2  = 2 * |r_f - r_o| / d,  r = sum R_n |x - x_n| / sum R_n over the objects, R_n the volume and x_n the weighted centroid;
      S   = (V_f - V_o) / (0.5 * (V_f + V_o)),  V = sum R_n * (R_n / w(peak_n)) / sum R_n;  L = L1 + L2.
    NaN where a side has no object or no volume; where a side has more objects than table rows the entries that need the objects
    (S, L2, L) are NaN rather than silently partial."""
    if 'volume' not in res:
        raise ValueError('sal: the result has no exact sums (Objects(sums=True))')
    t = int(threshold)
    if not 0 <= t < len(res['thresholds']):
        raise ValueError('sal: threshold index outside 0 ... %d' % (len(res['thresholds']) - 1))
    n_y, n_x = res['grid']
    d = float(np.sqrt(np.float64(n_x * n_x + n_y * n_y))) if d is None else float(d)
    if not d > 0.0:
        raise ValueError('sal: d must be positive')
    n_max = res['volume'].shape[-1]
    Df, xf, yf, rf, Vf = _sal_side(res, t, n_max, res['weight'])
    Do, xo, yo, ro, Vo = _sal_side(res['observed'], t, n_max, res['weight'])
    with np.errstate(invalid='ignore', divide='ignore'):
        A = (Df - Do) / (0.5 * (Df + Do))
        dx, dy = xf - xo, yf - yo
        L1 = np.sqrt(dx * dx + dy * dy) / d
        L2 = 2.0 * np.abs(rf - ro) / d
        S = (Vf - Vo) / (0.5 * (Vf + Vo))
    return {'S': S, 'A': A, 'L': L1 + L2, 'L1': L1, 'L2': L2}


def _match_side(res, threshold, who):
    if 'pieces' not in res:
        raise ValueError('%s: the result has no match (Objects(match=True))' % who)
    t = int(threshold)
    if not 0 <= t < len(res['thresholds']):
        raise ValueError('%s: threshold index outside 0 ... %d' % (who, len(res['thresholds']) - 1))
    return t


def pairs(res, block, threshold=0):
    """The distinct (forecast, observed) pairs of block `block` at threshold index `threshold` from a result with the match, sorted
    ascending: {'forecast', 'observed', 'area', 'sum_x', 'sum_y', 'pieces': int64 [n_pairs]}, the sums over the pair's pieces and
    their count.  ValueError when n_pieces > max_pieces: a partial fold is not returned."""
    t = _match_side(res, threshold, 'pairs')
    pc = res['pieces']
    b = int(block)
    n, rows = int(np.asarray(pc['n_pieces'])[b, t]), np.asarray(pc['area']).shape[-1]
    if n > rows:
        raise ValueError('pairs: %d pieces, %d rows (max_pieces): a partial fold is not returned' % (n, rows))
    f, o = np.asarray(pc['forecast'])[b, t, :n].astype(_I64), np.asarray(pc['observed'])[b, t, :n].astype(_I64)
    key, inverse = np.unique(f * (MAX_OBJECTS + 1) * 16 + o, return_inverse=True)        # (numbers are below 2^20 cells)
    inverse = inverse.reshape(-1)
    out = {'forecast': key // ((MAX_OBJECTS + 1) * 16), 'observed': key % ((MAX_OBJECTS + 1) * 16)}
    for k in ('area', 'sum_x', 'sum_y'):
        out[k] = np.bincount(inverse, weights=np.asarray(pc[k])[b, t, :n].astype(np.float64), minlength=key.size).astype(_I64)
    out['pieces'] = np.bincount(inverse, minlength=key.size).astype(_I64)
    return out


def match(res, threshold=0):
    """Per block and object of either side the partner with the largest pair area, and that area, from a result with the match at
    threshold index `threshold`: {'partner', 'area': int64 [n_blocks, max_objects] for the forecast objects (the partner is an
    observed object's number), 'observed_partner', 'observed_area' likewise for the observed objects against every block}.  Ties
    go to the smallest number; 0 means none (and the rows without an object).  -1 throughout for a block whose pieces overflowed.
    Partners beyond max_objects are named; objects beyond it have no row."""
    t = _match_side(res, threshold, 'match')
    n_blocks, rows = np.asarray(res['covered']).shape[0], np.asarray(res['covered']).shape[-1]
    out = {k: np.zeros((n_blocks, rows), dtype=_I64) for k in ('partner', 'area', 'observed_partner', 'observed_area')}
    for b in range(n_blocks):
        if int(np.asarray(res['pieces']['n_pieces'])[b, t]) > np.asarray(res['pieces']['area']).shape[-1]:
            for k in out:
                out[k][b] = -1
            continue
        p = pairs(res, b, t)
        for mine, other, kp, ka in (('forecast', 'observed', 'partner', 'area'), ('observed', 'forecast', 'observed_partner', 'observed_area')):
            # ascending area, then descending partner: the last entry of an object is its largest pair with the smallest number
            order = np.lexsort((-p[other], p['area'], p[mine]))
            who, area, partner = p[mine][order], p['area'][order], p[other][order]
            last = np.flatnonzero(np.append(who[1:] != who[:-1], True)) if who.size else np.zeros(0, dtype=_I64)
            ok = who[last] <= rows
            out[kp][b, who[last][ok] - 1], out[ka][b, who[last][ok] - 1] = partner[last][ok], area[last][ok]
    return out


def contingency(res, threshold=0, min_cover=0.0):
    """Object hits, misses and false alarms of every block against the observed map from a result with the match, at threshold
    index `threshold`: an observed object with covered_observed > min_cover * area is a hit, otherwise a miss; a forecast object
    with covered <= min_cover * area is a false alarm.  {'hits', 'misses', 'false_alarms': int64 [n_blocks], 'pod' = hits /
    (hits + misses), 'far' = false_alarms / (hits + false_alarms), 'csi' = hits / (hits + misses + false_alarms): float64, NaN
    for 0 / 0}.  From `covered` alone, so valid when the pieces overflow; where a side has more objects than table rows the block's
    counts are -1 and its scores NaN rather than silently partial."""
    t = _match_side(res, threshold, 'contingency')
    min_cover = float(min_cover)
    if not 0.0 <= min_cover < 1.0:
        raise ValueError('contingency: min_cover must lie in [0, 1)')
    cov, cov_o = np.asarray(res['covered'])[:, t].astype(np.float64), np.asarray(res['covered_observed'])[:, t].astype(np.float64)
    area, area_o = np.asarray(res['area'])[:, t].astype(np.float64), np.asarray(res['observed']['area'])[t].astype(np.float64)
    rows = area.shape[-1]
    hits = ((area_o > 0) & (cov_o > min_cover * area_o)).sum(axis=-1).astype(_I64)
    misses = ((area_o > 0) & ~(cov_o > min_cover * area_o)).sum(axis=-1).astype(_I64)
    alarms = ((area > 0) & (cov <= min_cover * area)).sum(axis=-1).astype(_I64)
    bad = (np.asarray(res['n_objects'])[:, t] > rows) | (int(np.asarray(res['observed']['n_objects'])[t]) > rows)
    with np.errstate(invalid='ignore', divide='ignore'):
        h, m, f = hits.astype(np.float64), misses.astype(np.float64), alarms.astype(np.float64)
        pod, far, csi = h / (h + m), f / (h + f), h / (h + m + f)
    out = {'hits': np.where(bad, -1, hits), 'misses': np.where(bad, -1, misses), 'false_alarms': np.where(bad, -1, alarms)}
    out.update(pod=np.where(bad, np.nan, pod), far=np.where(bad, np.nan, far), csi=np.where(bad, np.nan, csi))
    return out


def _track_side(res, threshold, who):
    if 'track' not in res:
        raise ValueError('%s: the result has no track (Objects(track=True))' % who)
    t = int(threshold)
    if not 0 <= t < len(res['thresholds']):
        raise ValueError('%s: threshold index outside 0 ... %d' % (who, len(res['thresholds']) - 1))
    return t


def links(res, pair, threshold=0, min_cover=0.0):
    """The distinct (earlier, later) object pairs of pair `pair` (block `pair` against block `pair` + 1) at threshold index
    `threshold` from a result with the track, sorted ascending: {'earlier', 'later', 'area', 'sum_x', 'sum_y', 'pieces': int64
    [n_links]} -- `pairs` applied to the track's pieces: the overlap area per link, after the shift, in the later block's frame.
    With `min_cover` > 0 the links whose area is below min_cover * min(area of the earlier object, area of the later one) are
    left out; the areas come from the table rows, so a link that names an object beyond max_objects is then a ValueError.
    ValueError when n_pieces > max_track_pieces: a partial fold is not returned."""
    t = _track_side(res, threshold, 'links')
    tr = res['track']
    p = int(pair)
    if not 0 <= p < np.asarray(tr['n_pieces']).shape[0]:
        raise ValueError('links: pair outside 0 ... %d' % (np.asarray(tr['n_pieces']).shape[0] - 1))
    min_cover = float(min_cover)
    if not 0.0 <= min_cover <= 1.0:
        raise ValueError('links: min_cover must lie in [0, 1]')
    pc = np.asarray(tr['pieces'])
    n, rows = int(np.asarray(tr['n_pieces'])[p, t]), pc.shape[-2]
    if n > rows:
        raise ValueError('links: %d pieces, %d rows (max_track_pieces): a partial fold is not returned' % (n, rows))
    named = {'n_pieces': tr['n_pieces'], 'area': pc[..., AREA], 'sum_x': pc[..., SUM_X], 'sum_y': pc[..., SUM_Y],
             'forecast': pc[..., FORECAST], 'observed': pc[..., OBSERVED]}
    f = pairs({'pieces': named, 'thresholds': res['thresholds']}, p, t)
    out = {'earlier': f['forecast'], 'later': f['observed'], 'area': f['area'], 'sum_x': f['sum_x'], 'sum_y': f['sum_y'], 'pieces': f['pieces']}
    if min_cover > 0.0 and out['area'].size:
        area = np.asarray(res['area'])
        if out['earlier'].max() > area.shape[-1] or out['later'].max() > area.shape[-1]:
            raise ValueError('links: min_cover needs the areas, and a link names an object beyond max_objects')
        least = np.minimum(area[p, t][out['earlier'] - 1], area[p + 1, t][out['later'] - 1]).astype(np.float64)
        keep = out['area'] >= min_cover * least
        out = {k: v[keep] for k, v in out.items()}
    return out


def tracks(res, threshold=0, min_cover=0.0):
    """Track ids of every object of every block at threshold index `threshold` from a result with the track.  THE RULE, statement by
    statement (blocks b = 0 ... B - 1, pairs p = 0 ... B - 2, objects by their numbers; an overlap is the area of a link of
    `links(res, p, threshold, min_cover)`, so overlaps below min_cover * min(area, area) do not count):
      1. The objects 1 ... n of block 0 open the tracks 1 ... n, in object order; birth 0, parent 0.
      2. For pair p, the predecessor of a later object is the earlier object with the largest overlap with it; ties go to the
         smallest number.  A later object without an overlap has none.
      3. Of the later objects that share a predecessor, the one with the largest overlap with it (ties: the smallest number)
         INHERITS the predecessor's track.
      4. The other later objects, in ascending order of their numbers, open new tracks with birth p + 1: those with a predecessor
         with `parent` = the predecessor's track (a split), those without with parent 0.
      5. An earlier object none of whose overlaps inherits ends its track there.  If it overlapped anything, `merged_into` of its
         track is the track of the later object it overlaps most (ties: the smallest number): a merge.
      6. `death` of a track is the last block that holds an object of it (B - 1 for the tracks that reach the end of the call).
    Returns {'track_id': [int64 [n_objects of block b] per block], 'inherited': [int64 [n, 2] (earlier, later) per pair: the
    links of statement 3], 'birth', 'death', 'parent', 'merged_into': int64 [n_tracks], entry k - 1 of track k, 0 = none}.
    ValueError when a needed n_pieces exceeds max_track_pieces: the links would be incomplete."""
    t = _track_side(res, threshold, 'tracks')
    n_obj = np.asarray(res['n_objects'])[:, t].astype(_I64)
    B = n_obj.size
    ids = [np.zeros(int(n), dtype=_I64) for n in n_obj]
    ids[0][:] = np.arange(1, int(n_obj[0]) + 1)
    birth, parent, merged, death = [0] * int(n_obj[0]), [0] * int(n_obj[0]), [0] * int(n_obj[0]), [0] * int(n_obj[0])
    inherited = []
    for p in range(B - 1):
        L = links(res, p, t, min_cover)
        e, l, a = L['earlier'], L['later'], L['area']
        ne, nl = int(n_obj[p]), int(n_obj[p + 1])
        # 2. the predecessor: per later object the link with the largest area, then the smallest earlier number
        pred, pred_area = np.zeros(nl + 1, dtype=_I64), np.zeros(nl + 1, dtype=_I64)
        order = np.lexsort((-e, a, l))                    # ascending area, then descending earlier: the last entry of a later object
        last = np.flatnonzero(np.append(l[order][1:] != l[order][:-1], True)) if l.size else np.zeros(0, dtype=_I64)
        pred[l[order][last]], pred_area[l[order][last]] = e[order][last], a[order][last]
        # 3. the heir: per earlier object, among the later objects whose predecessor it is, the largest overlap, then the smallest number
        heir = np.zeros(ne + 1, dtype=_I64)
        for j in range(1, nl + 1):
            i = int(pred[j])
            if i and (heir[i] == 0 or pred_area[j] > pred_area[heir[i]]):
                heir[i] = j
        for i in range(1, ne + 1):
            if heir[i]:
                ids[p + 1][heir[i] - 1] = ids[p][i - 1]
        inherited.append(np.array([(i, int(heir[i])) for i in range(1, ne + 1) if heir[i]], dtype=_I64).reshape(-1, 2))
        # 4. everything else opens a track
        for j in range(1, nl + 1):
            if ids[p + 1][j - 1] == 0:
                birth.append(p + 1)
                parent.append(int(ids[p][pred[j] - 1]) if pred[j] else 0)
                merged.append(0)
                death.append(p + 1)
                ids[p + 1][j - 1] = len(birth)
        for k in ids[p + 1]:
            death[k - 1] = p + 1
        # 5. the earlier objects without an heir: the later object they overlap most, then the smallest number
        order = np.lexsort((-l, a, e))
        last = np.flatnonzero(np.append(e[order][1:] != e[order][:-1], True)) if e.size else np.zeros(0, dtype=_I64)
        for i, j in zip(e[order][last].tolist(), l[order][last].tolist()):
            if not heir[i]:
                merged[int(ids[p][i - 1]) - 1] = int(ids[p + 1][j - 1])
    as_array = lambda v: np.array(v, dtype=_I64)
    return {'track_id': ids, 'inherited': inherited, 'birth': as_array(birth), 'death': as_array(death), 'parent': as_array(parent),
            'merged_into': as_array(merged)}


def motion(res, threshold=0):
    """The motion between the blocks at threshold index `threshold` from a result with the track: {'shift': int32 [P, 2] (dy, dx),
    the shift of every pair; 'links': per pair {'earlier', 'later': int64 [n], 'displacement': float64 [n, 2] (dy, dx)}: per
    inherited link of `tracks` the later object's centroid minus the earlier one's, from the table rows' integer sums (sum / area);
    NaN where an object lies beyond max_objects}."""
    t = _track_side(res, threshold, 'motion')
    tk = tracks(res, t)
    area, sx, sy = [np.asarray(res[k])[:, t].astype(np.float64) for k in ('area', 'sum_x', 'sum_y')]
    rows = area.shape[-1]
    out = []
    for p, link in enumerate(tk['inherited']):
        e, l = link[:, 0], link[:, 1]
        d = np.full((e.size, 2), np.nan)
        ok = (e <= rows) & (l <= rows)
        ei, li = e[ok] - 1, l[ok] - 1
        d[ok, 0] = sy[p + 1][li] / area[p + 1][li] - sy[p][ei] / area[p][ei]
        d[ok, 1] = sx[p + 1][li] / area[p + 1][li] - sx[p][ei] / area[p][ei]
        out.append({'earlier': e, 'later': l, 'displacement': d})
    return {'shift': np.asarray(res['track']['shift'])[:, t].copy(), 'links': out}


def size_distribution(res, edges):
    """int64 [..., len(edges) - 1]: the objects of every (block, threshold) counted by area in the bins [edges[k], edges[k + 1])
    (ascending cell counts).  Only the objects in the table are counted (n_objects may exceed max_objects)."""
    edges = np.asarray(edges)
    if edges.ndim != 1 or edges.size < 2 or np.any(edges[1:] <= edges[:-1]):
        raise ValueError('edges: at least two strictly ascending cell counts')
    area = res['area']
    k = np.searchsorted(edges, area, side='right') - 1        # bin of every row; rows without an object have area 0
    ok = (area > 0) & (k >= 0) & (k < edges.size - 1)
    out = np.zeros(area.shape[:-1] + (edges.size - 1,), dtype=_I64)
    for j in range(edges.size - 1):
        out[..., j] = (ok & (k == j)).sum(axis=-1)
    return out


class Cells(object):
    """A scored composite of ONE sweep call WITH its object cells, as RadarOperator._run_rays takes a product ("How a
    product plugs into a sweep call"): a neighbourhood.Scores, to which it delegates, and behind a finishing call the
    cpol_objects that hangs on its cpol_fractions.  It keeps the composite's `name`."""
    name = 'composite'
    spectrum, model_var = True, None
    refuses = NB.Scores.refuses
    _OWN = ('n_objects', 'table', 'labels', 'volume', 'skipped', 'field', 'field_cells', 'n_pieces', 'pieces', 'covered',
            'track_correlation', 'track_shift', 'track_n_pieces', 'track_pieces', 'track_covered')
    _SUMS, _MATCH, _TRACK = _OWN[3:7], _OWN[7:10], _OWN[10:]

    def __init__(self, spec, observed=None, domain=None, keep_gates=False, phase=3, rays_per_block=0, distributed=False):
        if not isinstance(spec, Objects):
            raise ValueError('spec: a cosmo_pol_amd.objects.Objects, got %r' % (spec,))
        self.scores = NB.Scores(spec.fractions, observed, domain, keep_gates, phase, rays_per_block, distributed)
        self.spec, self.gates = spec, self.scores.gates
        self.o = self.om = self.ot = None

    def set_plane(self, gate_xy, plane_version=0, source=0):
        self.scores.set_plane(gate_xy, plane_version, source)

    phase = property(lambda self: self.scores.phase, lambda self, v: setattr(self.scores, 'phase', int(v)))
    rays_per_block = property(lambda self: self.scores.rays_per_block, lambda self, v: setattr(self.scores, 'rays_per_block', int(v)))
    maps = property(lambda self: self.scores.maps)

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        structs, keep = self.scores.attach(native, az, n_gates, n_members, doppler, spectrum, staged_vars, take)
        self.o = self.om = self.ot = None
        if not self.phase & 2:                    # (no cpol_fractions in this call: nothing to hang on)
            return structs, keep
        self.n_blocks = self.scores.n_blocks
        shifts = None
        if self.spec.track:                       # (the blocks must be times, and at least two: the library refuses one block too)
            if n_members is not None:
                raise ValueError('track: the blocks of an ensemble call are members, not times')
            if self.n_blocks < 2:
                raise ValueError('track: the call yields %d block; tracking needs at least two (rays_per_block, or a series of times)' % self.n_blocks)
            if self.spec.shifts is not None:
                shifts = shifts_of_call(self.spec, self.n_blocks)
        if scratch_bytes(self.spec, self.n_blocks) > MAX_SCRATCH_BYTES:
            what = ('the labelling scratch, the sums, the pieces and the track of %d blocks need' if self.spec.track else
                    'the labelling scratch, the sums and the pieces of %d blocks need' if self.spec.match else
                    'the labelling scratch and the sums of %d blocks need' if self.spec.sums else 'the labelling scratch of %d blocks needs')
            raise ValueError('objects: %s more than 1 GiB' % (what % self.n_blocks))
        self.o, okeep = native.Context.objects_struct(self.spec, self.scores.f, shifts)
        if self.spec.track:
            self.ot = okeep[0]                    # (the ObjectsTrack around everything: it takes the five arrays of the track)
            self.om = self.ot.m if self.spec.match else None
        elif self.spec.match:
            self.om = okeep[0]                    # (the ObjectsMatch around self.o: it takes the three arrays of the match)
        return structs, keep + okeep

    def arrays(self):
        # the maps and the scores, then the cells, in the sweep's own block: they ride the one copy
        out = self.scores.arrays()
        if self.phase & 2:
            spec, nt = self.spec, len(self.spec.thresholds)
            out = out + [('n_objects', np.uint32, (self.n_blocks + 1, nt)),
                         ('table', np.uint32, (self.n_blocks + 1, nt, spec.max_objects, WORDS))]
            if spec.labels:
                out.append(('labels', np.int32, (self.n_blocks + 1, nt, spec.n_y, spec.n_x)))
            if spec.sums:
                out += [('volume', np.float64, (self.n_blocks + 1, nt, spec.max_objects, 3)),
                        ('skipped', np.uint32, (self.n_blocks + 1, nt, spec.max_objects)),
                        ('field', np.float64, (self.n_blocks + 1, 3)), ('field_cells', np.uint32, (self.n_blocks + 1, 2))]
            if spec.match:
                out += [('n_pieces', np.uint32, (self.n_blocks, nt)), ('pieces', np.uint32, (self.n_blocks, nt, spec.max_pieces, WORDS)),
                        ('covered', np.uint32, (self.n_blocks, nt, 2, spec.max_objects))]
            if spec.track:
                P = self.n_blocks - 1
                if spec.max_shift is not None:
                    out.append(('track_correlation', np.uint32, (P, nt, 2 * spec.max_shift + 1, 2 * spec.max_shift + 1)))
                out += [('track_shift', np.int32, (P, nt, 2)), ('track_n_pieces', np.uint32, (P, nt)),
                        ('track_pieces', np.uint32, (P, nt, spec.max_track_pieces, WORDS)),
                        ('track_covered', np.uint32, (P, nt, 2, spec.max_objects))]
        return out

    def bind(self, path, address):
        if path in self._TRACK:
            setattr(self.ot, path[len('track_'):], address)
        elif path in self._MATCH:
            setattr(self.om, path, address)
        elif path in self._OWN:
            setattr(self.o, path, address)
        else:
            self.scores.bind(path, address)

    def bind_device(self, entry):
        # the scores' entries and 'n_objects' | 'table' | 'labels' | 'volume' | 'skipped' | 'field' | 'field_cells' | 'n_pieces' |
        # 'pieces' | 'covered' | 'track_correlation' | 'track_shift' | 'track_n_pieces' | 'track_pieces' | 'track_covered': device pointers
        rest = {}
        for k, ptr in entry.items():
            if k in self._OWN and self.phase & 2 and (k not in self._MATCH or self.spec.match) and (
                    k not in self._TRACK or (self.spec.track and (k != 'track_correlation' or self.spec.max_shift is not None))):
                self.bind(k, ptr)
            else:
                rest[k] = ptr
        self.scores.bind_device(rest)

    def finish(self, w, coords):
        n, table = w.pop('n_objects'), w.pop('table')
        labels = w.pop('labels') if self.spec.labels else None
        sums = [w.pop(k) for k in self._SUMS] if self.spec.sums else None
        match = [w.pop(k) for k in self._MATCH] if self.spec.match else None
        track = None
        if self.spec.track:
            track = [w.pop(k) if (k != 'track_correlation' or self.spec.max_shift is not None) else None for k in self._TRACK]
        out = self.scores.finish(w, coords)
        out['objects'] = result(self.spec, n, table, labels, sums, match, track)
        return out

    def join(self, parts, cat):
        """The chunks of an ensemble call: a block per member -> the blocks joined (the observed map's cells are the same in
        every chunk: the last one's stand); else the last call holds the pass."""
        out = self.scores.join(parts, cat)
        if self.rays_per_block:
            ob = [w['objects'] for w in parts]
            stacked = [k for k in ob[-1] if k not in ('observed', 'connectivity', 'min_area', 'thresholds', 'weight', 'grid', 'field', 'pieces',
                                                      'track')]      # (no track in an ensemble call: attach refuses it)
            out['objects'] = dict(ob[-1], **{k: cat([q[k] for q in ob]) for k in stacked})
            for nested in ('field', 'pieces'):
                if nested in ob[-1]:
                    out['objects'][nested] = {k: cat([q[nested][k] for q in ob]) for k in ob[-1][nested]}
        return out
