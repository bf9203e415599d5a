"""Sweep histograms (cpol_histogram): CFADs, joint counts and plain histograms of the per-gate fields of a call, counted on the
device.  This module states the rule in NumPy (`count`); include/cosmo_pol_amd.h states the same text, and the GPU tests
compare the kernel (cosmo_pol_amd/csrc/cpol_hist.inl) with `count` exactly: the counts are integers.

THE RULE
  Input      the per-gate fields of the call as the launch sequence leaves them: after the range scans and the sensitivity
             cut, censored gates NaN; n_rows rows of n_gates gates (n_rows = n_rays, or n_members * n_rays in an ensemble call).
  Fields     the ten of FIELDS, in that order.  The type T is float32, except RVEL: float64.
  Abscissa   field k has n_x[k] >= 1 bins between n_x[k] + 1 edges.  The caller gives the edges as float64 in the field's own
             linear units; they are rounded once to T and must then be finite and strictly ascending.  The bin of a value v is
             ix = #{ j : e[j] <= v }, compared in T, in 0 ... n_x + 1: bin 0 is underflow, bin n_x + 1 overflow.  This is
             np.searchsorted(e_T, v, side='right'): comparisons only, no arithmetic.  +-inf land in the outer bins by
             themselves; -0.0 on an edge at +0.0 lands at or above it, as IEEE <= says.
  Ordinate   optional, one per struct: none (code 0), 'heights' (1, float32), 'dist' (2, float32), field k (16 + k, its type),
             row v of model_vars (32 + v, float64; only where the call produces model_vars).  n_y >= 1 bins, n_y + 1 edges, the
             same rule: iy in 0 ... n_y + 1.  In an ensemble call without time blend the geometry arrays hold n_rays rows
             once: row r takes the ordinate of row r mod n_rays.
  Counting   a gate counts for field k iff v == v, and with an ordinate also y == y; a counting gate adds 1 to
             counts[k][block][iy][ix].
  Blocks     rays_per_block = 0: one histogram for all rows of the call.  Otherwise it must divide n_rows, and block b holds
             the rows [b * rpb, (b + 1) * rpb).
  Counts     uint64, [n_blocks][n_y + 2][n_x[k] + 2], or [n_blocks][n_x[k] + 2] without an ordinate.
  A pass     phase bit 0 begins (clears, then counts), bit 1 finishes (counts, then writes out), 0 only counts.  The calls of a
             pass may differ in n_rays, n_gates and geometry when rays_per_block == 0; with rays_per_block > 0 every call gives
             the same number of blocks.  The result is a sum of integers: it depends neither on how the pass is cut into calls
             nor on any order of addition.
  Limits     n_x[k] + 1 and n_y + 1 at most MAX_EDGES; (n_x[k] + 2) * (n_y + 2) at most MAX_CELLS cells per field;
             n_blocks * sum_k cells_k at most MAX_STATE_CELLS."""
import numpy as np

FIELDS = ('ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL')
MAX_EDGES = 1024                 # n + 1 of either axis
MAX_CELLS = 16384                # (n_x + 2) * (n_y + 2) of one field: its table as uint32 fits 64 KiB of LDS
MAX_STATE_CELLS = 1 << 27        # n_blocks * the cells of all requested fields: 1 GiB of state
STRETCH = 512                    # gates per workgroup of k_hist (HIST_STRETCH in cpol_hist.h; checked against the library)

ORD_NONE, ORD_HEIGHTS, ORD_DIST, ORD_FIELD, ORD_MODEL = 0, 1, 2, 16, 32


def dtype_of(name):
    """The type T of a field or ordinate by name (('model', name) included)."""
    if isinstance(name, tuple) or name == 'RVEL':
        return np.float64
    return np.float32


def _edges(e, dt, what):
    a = np.asarray(e, dtype=np.float64)
    if a.ndim != 1 or a.size < 2:
        raise ValueError('%s: at least two edges in a 1-D sequence' % what)
    if a.size > MAX_EDGES:
        raise ValueError('%s: at most %d edges' % (what, MAX_EDGES))
    if not np.all(np.isfinite(a)):
        raise ValueError('%s: an edge is NaN or infinite' % what)
    with np.errstate(over='ignore'):
        r = a.astype(dt)
    if not np.all(np.isfinite(r)):
        raise ValueError('%s: an edge is infinite after rounding to %s' % (what, np.dtype(dt).name))
    if not np.all(r[1:] > r[:-1]):
        raise ValueError('%s: the edges are not strictly ascending after rounding to %s' % (what, np.dtype(dt).name))
    return a, r


class Histogram(object):
    """What a histogram call counts: `fields` {field name: edges}, the optional `ordinate` (None, 'heights', 'dist', a field
    name or ('model', variable name)) with `ordinate_edges`.  Edges are float64 in the field's own linear units (db_edges
    makes them from dB).  ValueError for what the library refuses."""

    def __init__(self, fields, ordinate=None, ordinate_edges=None):
        if not isinstance(fields, dict) or not fields:
            raise ValueError('fields: a non-empty dict {field name: edges}')
        for k in fields:
            if k not in FIELDS:
                raise ValueError('unknown field %r (one of %s)' % (k, ', '.join(FIELDS)))
        self.fields = tuple(k for k in FIELDS if k in fields)
        self.given, self.edges = {}, {}
        for k in self.fields:
            self.given[k], self.edges[k] = _edges(fields[k], dtype_of(k), 'edges of %s' % k)
        if isinstance(ordinate, list):
            ordinate = tuple(ordinate)
        self.ordinate = ordinate
        self.ordinate_given = self.ordinate_edges = None
        if ordinate is None:
            if ordinate_edges is not None:
                raise ValueError('ordinate_edges without an ordinate')
        else:
            ok = ordinate in ('heights', 'dist') or ordinate in FIELDS or (
                isinstance(ordinate, tuple) and len(ordinate) == 2 and ordinate[0] == 'model' and isinstance(ordinate[1], str))
            if not ok:
                raise ValueError("ordinate: None, 'heights', 'dist', a field name or ('model', name), got %r" % (ordinate,))
            if ordinate_edges is None:
                raise ValueError('an ordinate needs ordinate_edges')
            self.ordinate_given, self.ordinate_edges = _edges(ordinate_edges, dtype_of(ordinate), 'ordinate_edges')
        for k in self.fields:
            if (len(self.edges[k]) + 1) * self.n_y_cells > MAX_CELLS:
                raise ValueError('%s: (n_x + 2) * (n_y + 2) = %d cells, at most %d' %
                                 (k, (len(self.edges[k]) + 1) * self.n_y_cells, MAX_CELLS))

    @property
    def n_y_cells(self):
        """n_y + 2, or 1 without an ordinate."""
        return 1 if self.ordinate is None else len(self.ordinate_edges) + 1

    @property
    def mask(self):
        return sum(1 << FIELDS.index(k) for k in self.fields)

    @property
    def cells(self):
        """The cells of one block: all requested fields."""
        return sum((len(self.edges[k]) + 1) * self.n_y_cells for k in self.fields)

    @property
    def key(self):
        return (tuple((k, self.edges[k].tobytes()) for k in self.fields), self.ordinate,
                None if self.ordinate is None else self.ordinate_edges.tobytes())

    def __eq__(self, other):
        return isinstance(other, Histogram) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        f = ', '.join('%s: %d bins' % (k, len(self.edges[k]) - 1) for k in self.fields)
        if self.ordinate is None:
            return 'Histogram({%s})' % f
        return 'Histogram({%s}, ordinate=%r: %d bins)' % (f, self.ordinate, len(self.ordinate_edges) - 1)


def db_edges(lo, hi, step):
    """Edges lo, lo + step, ... up to hi (dB) as linear float64 edges 10 ** (x / 10): a dBZ histogram of the linear field
    needs no logarithm on the device."""
    lo, hi, step = float(lo), float(hi), float(step)
    if not (step > 0.0 and hi > lo):
        raise ValueError('db_edges: hi > lo and step > 0')
    n = int(np.floor((hi - lo) / step + 1e-9))
    x = lo + step * np.arange(n + 1, dtype=np.float64)
    return 10.0 ** (x / 10.0)


def centers(edges):
    """The midpoints of the bins between `edges`."""
    e = np.asarray(edges, dtype=np.float64)
    return 0.5 * (e[1:] + e[:-1])


def n_blocks(n_rows, rays_per_block=0):
    rpb = int(rays_per_block)
    if rpb < 0 or (rpb and n_rows % rpb):
        raise ValueError('rays_per_block %r does not divide the %d rows of the call' % (rays_per_block, n_rows))
    return n_rows // rpb if rpb else 1


def shape(spec, field, n_rows=1, rays_per_block=0):
    """The shape of counts[field] for a call of n_rows rows."""
    nb = n_blocks(n_rows, rays_per_block)
    nx = len(spec.edges[field]) + 1
    return (nb, nx) if spec.ordinate is None else (nb, spec.n_y_cells, nx)


def _ordinate_of(per_gate, spec):
    o = spec.ordinate
    if isinstance(o, tuple):
        mv = per_gate['model_vars']
        if not isinstance(mv, dict) or o[1] not in mv:
            raise ValueError("count: per_gate['model_vars'] must be a dict holding %r" % (o[1],))
        return np.asarray(mv[o[1]])
    return np.asarray(per_gate[o])


def count(per_gate, spec, rays_per_block=0, n_rays=None, into=None):
    """The rule in NumPy.  per_gate: {name: array [..., n_gates]} for the fields of `spec` and its ordinate ('heights', 'dist',
    a field, or per_gate['model_vars'][name]); leading axes are flattened to rows.  An ordinate with fewer rows than the
    fields (n_rays of them: the geometry of an ensemble call) is taken row mod n_rays.  Returns {field: uint64 counts};
    `into` (a former result) continues a pass: the counts are added to it in place."""
    out = {} if into is None else into
    y = None
    for k in spec.fields:
        v = np.asarray(per_gate[k])
        if v.dtype != dtype_of(k):
            raise ValueError('count: %s must be %s' % (k, np.dtype(dtype_of(k)).name))
        ng = v.shape[-1]
        v = v.reshape(-1, ng)
        rows = v.shape[0]
        nb = n_blocks(rows, rays_per_block)
        rpb = rows // nb
        sh = shape(spec, k, rows, rays_per_block)
        if k not in out:
            out[k] = np.zeros(sh, dtype=np.uint64)
        if out[k].shape != sh or out[k].dtype != np.uint64:
            raise ValueError('count: into[%r] has shape %s, this call gives %s' % (k, out[k].shape, sh))
        ix = np.searchsorted(spec.edges[k], v, side='right')
        ok = v == v
        nx = len(spec.edges[k]) + 1
        if spec.ordinate is not None:
            if y is None:
                y = _ordinate_of(per_gate, spec)
                if y.dtype != dtype_of(spec.ordinate):
                    raise ValueError('count: the ordinate must be %s' % np.dtype(dtype_of(spec.ordinate)).name)
                y = y.reshape(-1, ng)
                iy = np.searchsorted(spec.ordinate_edges, y, side='right')
                oky = y == y
            if y.shape[0] != rows:
                ny_rows = y.shape[0] if n_rays is None else int(n_rays)
                if ny_rows != y.shape[0] or rows % ny_rows:
                    raise ValueError('count: the ordinate has %d rows, the fields %d' % (y.shape[0], rows))
                sel = np.arange(rows) % ny_rows
                iy_k, oky_k = iy[sel], oky[sel]
            else:
                iy_k, oky_k = iy, oky
            ok = ok & oky_k
            cell = iy_k * nx + ix
            per = spec.n_y_cells * nx
        else:
            cell = ix
            per = nx
        cell = cell + (np.arange(rows) // rpb)[:, None] * per
        add = np.bincount(cell[ok].ravel(), minlength=nb * per).astype(np.uint64)
        out[k] += add.reshape(sh)
    return out


def frequencies(counts):
    """The CFAD normalisation: each ordinate row (the last axis) divided by its own total over all n_x + 2 cells; NaN where
    that total is 0."""
    c = np.asarray(counts).astype(np.float64)
    tot = c.sum(axis=-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(tot > 0, c / tot, np.nan)


class Counts(object):
    """The histogram of ONE sweep call, as RadarOperator._run_rays takes a product ("How a product plugs into a
    sweep call"): this call's gates counted into the lane's running histogram.  `phase` and `rays_per_block` may be set anew
    between the calls of a pass; the counts arrive with a finishing call (phase bit 1)."""
    name = 'histogram'
    spectrum = True
    refuses = {'subbeams': 'histograms and composites do not share a call with superobservations, ensemble statistics, '
                           'spectrum moments or the sub-beam export',
               'groups': 'a histogram or composite call needs one group (cut the rays and fold the calls into one pass with '
                         'phase=)'}

    def __init__(self, spec, keep_gates=False, phase=3, rays_per_block=0, doppler=True, distributed=False):
        # what a histogram call refuses before it builds anything.  (Spaceborne geometry is refused by the ray calls
        # themselves: they take ground radars.)
        if not isinstance(spec, Histogram):
            raise ValueError('hist: a cosmo_pol_amd.histogram.Histogram, got %r' % (spec,))
        if distributed:
            raise NotImplementedError('histograms with a process group: sharding rays over ranks is not built')
        if ('RVEL' in spec.fields or spec.ordinate == 'RVEL') and not doppler:
            raise ValueError('histogram: RVEL needs a Doppler scheme')
        self.spec, self.gates, self.phase, self.rays_per_block = spec, bool(keep_gates), int(phase), int(rays_per_block)
        # an ordinate ('model', name): the library integrates the model variables for it, asked for or not
        self.model_var = spec.ordinate[1] if isinstance(spec.ordinate, tuple) else None

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        self.n_rows = len(az) * (n_members or 1)
        n_blocks(self.n_rows, self.rays_per_block)            # (ValueError: the library refuses the same)
        self.h, keep = native.Context.histogram_struct(
            self.spec, self.phase, self.rays_per_block,
            model_index=staged_vars.index(self.model_var) if self.model_var is not None else None)
        return {'histogram': self.h}, keep

    def arrays(self):
        # the counts, in the sweep's own block: they ride the one copy
        return ([(k, np.uint64, shape(self.spec, k, self.n_rows, self.rays_per_block)) for k in self.spec.fields]
                if self.phase & 2 else [])

    def bind(self, path, address):
        self.h.counts[FIELDS.index(path)] = address

    def bind_device(self, entry):         # {field: device pointer of its uint64 counts}
        for k, ptr in (entry.items() if self.phase & 2 else ()):
            self.bind(k, ptr)

    def finish(self, w, coords):
        return {'counts': w, 'edges': {k: self.spec.edges[k] for k in self.spec.fields},
                'ordinate_edges': self.spec.ordinate_edges}

    def join(self, parts, cat):
        """The chunks of an ensemble call: one histogram per member (rays_per_block set) -> the blocks joined; else the
        chunks were one pass and the last call holds its counts."""
        out = dict(parts[-1])
        if self.rays_per_block:
            out['counts'] = {k: cat([q['counts'][k] for q in parts]) for k in self.spec.fields}
        return out
