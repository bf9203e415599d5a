"""Object cells (cpol_objects): the connected components of the binary maps of a neighbourhood verification, numbered, with ten
integer attributes each, found on the device behind the scores.  This module states the rule in NumPy (`cells`);
include/cosmo_pol_amd.h states the same text, and the GPU tests compare the kernels (cosmo_pol_amd/csrc/cpol_obj.inl) with it
exactly: every attribute is a count, an integer sum, an integer extreme or a comparison.

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
  Not built  float sums over an object's cells (rain volume, weighted centroids, SAL's S and L2): the label map is delivered so
             that the host can form them.
  Limits     the labelling scratch, (n_blocks + 1) * n_thr * (2 * n_y * n_x + n_y) * 4 bytes, at most MAX_SCRATCH_BYTES."""
import numpy as np

from . import neighbourhood as NB

WORDS = 10
MAX_OBJECTS = 65535
MAX_SCRATCH_BYTES = 1 << 30
FIRST, AREA, SUM_X, SUM_Y, X0, X1, Y0, Y1, PEAK_CELL, PEAK_BITS = range(WORDS)

_U32, _I64 = np.uint32, np.int64


class Objects(object):
    """What a call with object cells finds: the cells of the binary maps of `fractions` (a neighbourhood.Fractions) under
    `connectivity` 4 or 8, those below `min_area` cells dropped, up to `max_objects` (1 ... 65535) table rows per source and
    threshold, with the label maps when `labels`.  ValueError for what the library refuses.  The Fractions is `fractions`; the
    properties the scored entry points read of a spec are its own."""

    def __init__(self, fractions, connectivity=4, min_area=1, max_objects=1024, labels=True):
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

    composite = property(lambda self: self.fractions.composite)
    thresholds = property(lambda self: self.fractions.thresholds)
    n_x = property(lambda self: self.fractions.n_x)
    n_y = property(lambda self: self.fractions.n_y)

    @property
    def key(self):
        return (self.fractions.key, self.connectivity, self.min_area, self.max_objects, self.labels)

    def __eq__(self, other):
        return isinstance(other, Objects) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return 'Objects(%r, connectivity=%d, min_area=%d, max_objects=%d, labels=%r)' % (
            self.fractions, self.connectivity, self.min_area, self.max_objects, self.labels)


def scratch_bytes(spec, blocks):
    """The bytes of the labelling scratch of `blocks` blocks and the observation (cpol_obj.h)."""
    return (int(blocks) + 1) * len(spec.thresholds) * (2 * spec.n_y * spec.n_x + spec.n_y) * 4


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


def result(spec, n_objects, table, labels=None):
    """The output arrays named.  n_objects [n_blocks + 1, n_thr], table [n_blocks + 1, n_thr, max_objects, WORDS], labels
    [n_blocks + 1, n_thr, n_y, n_x] or None -> {'n_objects': uint32 [n_blocks, n_thr], 'first' | 'area' | 'sum_x' | 'sum_y' |
    'peak_cell': uint32 [n_blocks, n_thr, max_objects], 'bbox': uint32 [..., 4] (x0, x1, y0, y1), 'peak': float32 [...],
    'labels': int32 [n_blocks, n_thr, n_y, n_x] (when given), 'observed': the same of the observed map without the leading
    axis, 'connectivity', 'min_area', 'thresholds'}."""
    def named(n, tb, lb):
        out = {'n_objects': n, 'first': tb[..., FIRST], 'area': tb[..., AREA], 'sum_x': tb[..., SUM_X], 'sum_y': tb[..., SUM_Y],
               'bbox': tb[..., X0:Y1 + 1], 'peak': tb[..., PEAK_BITS].view(np.float32),     # (views all: a pinned call fills them later)
               'peak_cell': tb[..., PEAK_CELL]}
        if lb is not None:
            out['labels'] = lb
        return out
    out = named(n_objects[:-1], table[:-1], None if labels is None else labels[:-1])
    out['observed'] = named(n_objects[-1], table[-1], None if labels is None else labels[-1])
    out.update(connectivity=spec.connectivity, min_area=spec.min_area, thresholds=spec.thresholds)
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
    returns ('labels' only with spec.labels)."""
    F, O, m, o = binary_maps(spec.fractions, plane_maps, observed, domain)
    n_blocks, n_thr = F.shape[:2]
    n = np.zeros((n_blocks + 1, n_thr), dtype=_U32)
    table = np.zeros((n_blocks + 1, n_thr, spec.max_objects, WORDS), dtype=_U32)
    labels = np.zeros((n_blocks + 1, n_thr) + o.shape, dtype=np.int32)
    for s in range(n_blocks + 1):
        for t in range(n_thr):
            binary, values = (F[s, t], m[s]) if s < n_blocks else (O[t], o)
            n[s, t], table[s, t], labels[s, t] = cells_of_map(binary, values, spec.connectivity, spec.min_area, spec.max_objects)
    return result(spec, n, table, labels if spec.labels else None)


def centroids(res):
    """float64 [..., max_objects, 2] (x, y): the centroids of the objects in GRID coordinates, sum / area plus the half cell (cell
    ix covers [ix, ix + 1)); NaN in the rows without an object.  `res`: what `result` returns, or its 'observed'."""
    area = res['area'].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        c = np.stack([res['sum_x'] / area + 0.5, res['sum_y'] / area + 0.5], axis=-1)
    return np.where((area > 0)[..., None], c, np.nan)


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
    _OWN = ('n_objects', 'table', 'labels')

    def __init__(self, spec, observed=None, domain=None, keep_gates=False, phase=3, rays_per_block=0, distributed=False):
        if not isinstance(spec, Objects):
            raise ValueError('spec: a cosmo_pol_amd.objects.Objects, got %r' % (spec,))
        self.scores = NB.Scores(spec.fractions, observed, domain, keep_gates, phase, rays_per_block, distributed)
        self.spec, self.gates = spec, self.scores.gates
        self.o = None

    def set_plane(self, gate_xy, plane_version=0, source=0):
        self.scores.set_plane(gate_xy, plane_version, source)

    phase = property(lambda self: self.scores.phase, lambda self, v: setattr(self.scores, 'phase', int(v)))
    rays_per_block = property(lambda self: self.scores.rays_per_block, lambda self, v: setattr(self.scores, 'rays_per_block', int(v)))
    maps = property(lambda self: self.scores.maps)

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        structs, keep = self.scores.attach(native, az, n_gates, n_members, doppler, spectrum, staged_vars, take)
        self.o = None
        if not self.phase & 2:                    # (no cpol_fractions in this call: nothing to hang on)
            return structs, keep
        self.n_blocks = self.scores.n_blocks
        if scratch_bytes(self.spec, self.n_blocks) > MAX_SCRATCH_BYTES:
            raise ValueError('objects: the labelling scratch of %d blocks needs more than 1 GiB' % self.n_blocks)
        self.o, okeep = native.Context.objects_struct(self.spec, self.scores.f)
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
        return out

    def bind(self, path, address):
        if path in self._OWN:
            setattr(self.o, path, address)
        else:
            self.scores.bind(path, address)

    def bind_device(self, entry):
        # the scores' entries and 'n_objects' | 'table' | 'labels': device pointers
        rest = {}
        for k, ptr in entry.items():
            if k in self._OWN and self.phase & 2:
                self.bind(k, ptr)
            else:
                rest[k] = ptr
        self.scores.bind_device(rest)

    def finish(self, w, coords):
        n, table = w.pop('n_objects'), w.pop('table')
        labels = w.pop('labels') if self.spec.labels else None
        out = self.scores.finish(w, coords)
        out['objects'] = result(self.spec, n, table, labels)
        return out

    def join(self, parts, cat):
        """The chunks of an ensemble call: a block per member -> the blocks joined (the observed map's cells are the same in
        every chunk: the last one's stand); else the last call holds the pass."""
        out = self.scores.join(parts, cat)
        if self.rays_per_block:
            ob = [w['objects'] for w in parts]
            stacked = [k for k in ob[-1] if k not in ('observed', 'connectivity', 'min_area', 'thresholds')]
            out['objects'] = dict(ob[-1], **{k: cat([q[k] for q in ob]) for k in stacked})
        return out
