"""Gridded composites (cpol_composite): the column maximum, the lowest gate and echo-top heights of the per-gate fields of a
call on a radar-centred map, reduced on the device.  This module states the rule in NumPy (`compose`, `finish`);
include/cosmo_pol_amd.h states the same text, and the GPU tests compare the kernels (cosmo_pol_amd/csrc/cpol_comp.inl) with it
exactly: every result is a maximum, a minimum or a count of integers.

THE RULE
  Input      the per-gate fields of the call as the launch sequence leaves them: after the range scans and the sensitivity
             cut, censored gates NaN; n_rows rows of n_gates gates (n_rows = n_rays, or n_members * n_rays in an ensemble
             call).  With them `dist` (float32, ground distance of the central sub-beam) and `heights` (float32) of the same
             call, and per ray two float64 numbers ray_sin[r], ray_cos[r] given by the caller: np.sin(np.deg2rad(az)),
             np.cos(np.deg2rad(az)) (`ray_tables`).  The library computes no trigonometric function for this product.
             Geometry arrays that hold n_rays rows once are read at g mod (n_rays * n_gates), the per-ray pair at row mod n_rays.
  Plane      radar-centred, east x and north y: x = float64(dist) * ray_sin, y = float64(dist) * ray_cos, one float64
             multiplication each.
  Grid       n_x + 1 and n_y + 1 float64 edges, finite and strictly ascending, at most MAX_EDGES per axis.
             ix = #{ j : ex[j] <= x } - 1 = np.searchsorted(ex, x, side='right') - 1, likewise iy: comparisons alone.  The gate
             lies in the grid iff 0 <= ix < n_x and 0 <= iy < n_y; there are no under- or overflow cells (a gate on the last
             edge is outside), and a gate outside the grid does not count.
  Slab       optional, [h_lo, h_hi): both bounds rounded once to float32, the test h_lo <= h and h < h_hi in float32.  Without a
             slab every height counts.
  Fields     the nine float32 fields of FIELDS, bit k as in histogram.FIELDS.  RVEL is float64 and is refused.
  Counting   a gate counts for field k iff v == v, dist == dist, h == h, it lies in the grid and it lies in the slab.
  Key        of a float32 with bits b: key = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000), a total order
             -inf < ... < -0.0 < +0.0 < ... < +inf.  Keys 0 and 0xFFFFFFFF belong to NaN bit patterns: no counting value
             produces them, and they mark an empty cell.
  Products   per requested field, the same for all fields of a spec:
             'max'       planes max, height_of_max: one uint64 per cell, the MAXIMUM of key(v) << 32 | key(h) over the
                         counting gates; ties in the value go to the greater height.
             'lowest'    planes lowest, height_of_lowest: one uint64 per cell, the MINIMUM of key(h) << 32 | key(v); ties in
                         the height go to the smaller value.
             'echo_top'  planes echo_top_0 ...: 1 to MAX_THRESHOLDS thresholds per field in the field's own linear units, each
                         rounded once to float32; per plane one uint32 per cell, the maximum of key(h) over the counting gates
                         with v >= t.
             count       always: uint64 per cell and field, the number of counting gates.
  Blocks     rays_per_block = 0: one map of all rows of the call.  Otherwise it must divide n_rows, and block b holds the rows
             [b * rpb, (b + 1) * rpb): rpb = n_rays one map per member.
  A pass     a begin sets the max states to 0, the min states to all ones and the counts to 0.  With rays_per_block == 0 the
             calls of a pass may differ in n_rays, n_gates and geometry: the sweeps of a volume fold into one composite.  The
             result depends neither on how the pass is cut into calls nor on any order.
  Outputs    per requested field float32 [n_blocks][n_planes][n_y][n_x], the planes in the order max, height_of_max, lowest,
             height_of_lowest, echo_top_0 ..., planes not requested absent, empty cells NaN; count uint64
             [n_blocks][n_requested_fields][n_y][n_x], the fields ascending.
  Limits     at most MAX_EDGES edges per axis; the state of all blocks and fields at most MAX_STATE_BYTES; fewer than 2^31
             workgroups.

NETWORK COMPOSITES: several radars on one geographic or model grid.  Everything above stays as it is.
  Plane      'radar' (CPOL_COMP_PLANE_RADAR = 0) is the plane above.  On a gate plane (CPOL_COMP_PLANE_GATES = 1) the caller
             supplies per-gate coordinates gate_x, gate_y, float64 [n_rays * n_gates], read at g mod (n_rays * n_gates) exactly
             as `dist` is: x = gate_x[g], y = gate_y[g], no multiplication; `dist` is not read and no azimuth is needed.  A gate
             counts iff v == v, h == h, x == x, y == y, it lies in the grid and it lies in the slab; the cell search is the same
             comparisons alone.  The library still computes no trigonometric function: every projection is the caller's
             (`plane_xy`: longitude and latitude, the rotated grid of the model, or any callable).
  Source     every call carries a number `source`, 0 ... 254, e.g. the index of its radar.  With the product 'source'
             (CPOL_COMP_SOURCE = 16; it needs 'max' or 'lowest') the plane source_of_max holds the smallest `source` among the
             counting gates of the whole pass whose key(v) << 32 | key(h) equals the cell's final MAX state, source_of_lowest the
             same for the LOWEST state: float32 (exact small integers), empty cells NaN.  The planes are then max,
             height_of_max, source_of_max, lowest, height_of_lowest, source_of_lowest, echo_top_0 ....  The definition is
             symmetric in the calls: the pass still depends neither on how it is cut into calls nor on their order.  The state
             gains one source byte per cell, block and product (begin value 255) and a per-call scratch state.

HEIGHT LAYERS AND THE COLUMN: a stack of CAPPIs in one pass, and column integrals such as VIL.  Without `z_edges` everything above
stays as it is.
  Layers     z_edges: 2 ... MAX_Z_EDGES height edges in metres, each rounded once to float32, strictly ascending after the
             rounding and not NaN: n_z = 1 ... MAX_LAYERS layers.  A gate that counts above counts in layer l iff
             ez[l] <= h < ez[l + 1] in float32: a gate on the last edge is outside, as on the x and y axes, and a gate below the
             first edge or at or above the last counts nowhere.  Per (block, layer, cell) the state is the MAX state and the
             count of above.  Planes max, height_of_max: float32 [n_blocks, n_z, n_y, n_x]; count uint64 likewise.  With layers
             height_range (the first and last edge are the slab), 'lowest', 'echo_top' and 'source' are refused; several radars
             still fold into one pass on a gate plane, `source` stays 0.
  Column     the product 'column' (CPOL_COMP_COLUMN = 64) needs layers and 'max'.  Per field a table: table_v, float32
             breakpoints in the field's linear units, 2 ... MAX_TABLE of them, finite and strictly ascending; table_f, float64
             values at the breakpoints, finite.  For a layer whose maximum v exists: i = searchsorted(table_v, v, 'right') - 1;
             i < 0: f = 0.0; i >= n - 1: f = table_f[n - 1] (the cap; +inf takes it); else
             t = (float64(v) - float64(tv[i])) / (float64(tv[i + 1]) - float64(tv[i])), f = tf[i] + t * (tf[i + 1] - tf[i]),
             every operation ONE float64 operation.  C = sum over l ascending from +0.0 of f_l * dz_l with
             dz_l = float64(ez[l + 1]) - float64(ez[l]): one thread's loop, no order of the hardware enters.
  Gaps       an empty layer: 'zero' adds nothing; 'hold': an empty layer with a counting layer below it and a counting layer
             above it in the same cell takes the f of the nearest counting layer below; empty layers below the lowest or above
             the highest counting layer add nothing.  A cell with no counting layer is NaN.
  Outputs    column[field] float64 [n_blocks, n_y, n_x]; column_layers[field] uint8 [n_blocks, n_y, n_x], the layers that
             contributed (under 'hold' the held ones included).

SUM: the exact sum of the counting gates' weights per (block, layer, cell), for the cell MEAN and for rain accumulations (the
product 'sum', CPOL_COMP_SUM = 256, and the struct cpol_composite_sums).  Everything above stays as it is.
  1.  A gate counts for field k exactly as above: the same cell search, slab, layers, blocks and pass.
  2.  The summand of a counting gate is w = v when field k has no weight table.  With a table (table_v float32, table_f float64)
      it is w = float32(f(v)), f the piecewise-linear function of the column table above: 0 below the table, the last value at
      and above its end, every operation one float64 operation, then ONE rounding to float32 (obj_weight in cpol_obj.h,
      objects.weight_of).  The table conditions are those of the column table: 2 ... 1024 breakpoints, finite, strictly
      ascending in float32, finite values; no monotonicity is demanded of the values.
  3.  Per (block, layer, cell) `sum` is the EXACT sum of the finite w, rounded ONCE to float64 with ties to even: math.fsum of
      the summands.  +0.0 when the exact sum is zero, NaN when no gate was summed.
  4.  Per (block, layer, cell) `sum_skipped` (uint32) is the number of counting gates with w = +-inf.  Such a gate is not
      summed, and it still counts in `count`.
  5.  The mean is sum / (count - sum_skipped): one float64 division, formed on the host (`mean_of`), NaN where the divisor
      is 0.
  6.  Nothing depends on the order of the gates, the lane form, the block cut or how the pass is cut into calls.
  How        a finite float32 is +-M * 2 ** (E - 150) with E in 1 ... 254 and M < 2 ** 24 (objects.split).  The state gains per
             field and (block, layer, cell) a row of SUM_BINS signed 64-bit bins and one uint32 skipped word; bin E >> 3 takes
             +-M << (E & 7), an INTEGER addition, and `finish` folds a row into one Python integer and rounds it once
             (objects.round_scaled).  Integer additions commute: no order enters.
  No overflow  a term is below 2 ** 31 in magnitude, so a bin cannot wrap while fewer than 2 ** 32 gates fold into one block of
             a pass; the library refuses the call that would take a block beyond SUM_MAX_GATES.
  Beside     'sum' stands beside at least one of 'max', 'lowest', 'echo_top'; 'sum' with 'source' is refused; with layers it
             gives a 3-D grid of sums.  Not built: 'sum' alone, 'sum' with 'source', sums of RVEL, means in dB, a
             carry-normalising kernel for passes beyond 2 ** 32 gates."""
import numpy as np

from .histogram import Counts

FIELDS = ('ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V')
PRODUCTS = ('max', 'lowest', 'echo_top')             # bit 0, 1, 2 of cpol_composite.products
SOURCE, SOURCE_BIT = 'source', 16                    # CPOL_COMP_SOURCE (8 is no product and stays refused)
COLUMN, COLUMN_BIT = 'column', 64                    # CPOL_COMP_COLUMN (32 is no product and stays refused)
SUM, SUM_BIT = 'sum', 256                            # CPOL_COMP_SUM (128 is no product and stays refused)
SUM_BINS = 32                                        # COMP_SUM_BINS: the int64 bins of a cell's row
SUM_MAX_GATES = (1 << 32) - 1                        # COMP_SUM_MAX_GATES: the gates one block of a pass may fold
GAPS = ('zero', 'hold')                              # cpol_composite.gaps
MAX_LAYERS = 64                  # n_z; z_edges holds n_z + 1 values
MAX_Z_EDGES = MAX_LAYERS + 1
MAX_TABLE = 1024                 # breakpoints of a column table
NO_SOURCE = 255                                      # the begin value of a source byte; sources are 0 ... 254
PLANES = ('radar', 'geographic', 'model')            # or a callable f(lats, lons) -> (x, y): see plane_xy
MAX_EDGES = 1024                 # n + 1 of either axis
MAX_THRESHOLDS = 4               # echo-top planes of one field
MAX_STATE_BYTES = 1 << 30        # the state of all blocks and fields
STRETCH = 1024                   # gates per workgroup of k_comp (COMP_STRETCH in cpol_comp.h; checked against the library)

_U32, _U64 = np.uint32, np.uint64
_LOW_EMPTY = _U64(0xFFFFFFFFFFFFFFFF)


def key32(a):
    """The ordered key (uint32) of float32 values."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(_U32)
    return b ^ np.where(b >> _U32(31), _U32(0xFFFFFFFF), _U32(0x80000000)).astype(_U32)


def unkey32(k):
    """The float32 values of ordered keys: the inverse of key32."""
    k = np.ascontiguousarray(k, dtype=_U32)
    return (k ^ np.where(k >> _U32(31), _U32(0x80000000), _U32(0xFFFFFFFF)).astype(_U32)).view(np.float32)


def _edges(e, what):
    a = np.array(e, dtype=np.float64)
    if a.ndim != 1 or a.size < 2:
        raise ValueError('%s: at least two edges in a 1-D sequence' % what)
    if a.size > MAX_EDGES:
        raise ValueError('%s: at most %d edges' % (what, MAX_EDGES))
    if not np.all(np.isfinite(a)):
        raise ValueError('%s: an edge is NaN or infinite' % what)
    if not np.all(a[1:] > a[:-1]):
        raise ValueError('%s: the edges are not strictly ascending' % what)
    return a


def _f32(v):
    with np.errstate(over='ignore'):
        return np.float32(v)


def _table(table, what):
    """(table_v float32, table_f float64) of a weight table under the conditions of the column table."""
    try:
        tv, tf = table
        tvg = np.array(tv, dtype=np.float64).reshape(-1)
        tf = np.array(tf, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError('%s: (table_v, table_f), got %r' % (what, table))
    if not 2 <= tvg.size <= MAX_TABLE:
        raise ValueError('%s: 2 ... %d breakpoints, got %d' % (what, MAX_TABLE, tvg.size))
    if tf.size != tvg.size:
        raise ValueError('%s: %d breakpoints and %d values' % (what, tvg.size, tf.size))
    with np.errstate(over='ignore'):
        tv32 = tvg.astype(np.float32)
    if not (np.all(np.isfinite(tv32)) and np.all(np.isfinite(tf))):
        raise ValueError('%s: a breakpoint or a value is NaN or infinite' % what)
    if not np.all(tv32[1:] > tv32[:-1]):
        raise ValueError('%s: the breakpoints are not strictly ascending in float32' % what)
    return tv32, tf


class Composite(object):
    """What a composite call reduces: `fields` (names out of FIELDS), the float64 `x_edges` (east) and `y_edges` (north) of the
    radar-centred grid in metres (`grid` makes a uniform one), `products` out of PRODUCTS, `thresholds` for 'echo_top' ({field:
    1 ... 4 thresholds in the field's own linear units}, or one sequence for every field; `from_db` makes them from dBZ) and the
    optional `height_range` (h_lo, h_hi): only gates with h_lo <= height < h_hi count.  A slab around a nominal height with
    'max' alone is a pseudo-CAPPI.  `plane`: 'radar' (the default: radar-centred metres), 'geographic' (x_edges longitudes,
    y_edges latitudes, degrees), 'model' (rotated longitudes and latitudes of the staged model's grid) or a callable
    f(lats, lons) -> (x, y): on every plane but 'radar' the sweep calls hand the library per-gate coordinates made by
    `plane_xy`, and several radars may fold into one pass.  The product 'source' (beside 'max' or 'lowest') adds the planes
    source_of_max / source_of_lowest: which call's `source` supplied the cell.  `z_edges`: 2 ... 65 height edges in metres:
    the planes gain a layer axis ([n_blocks, n_z, n_y, n_x]: a stack of CAPPIs in one pass); with the product 'column' and
    `column` = {field: (table_v, table_f)} (`vil_table` makes the one of VIL) the result gains the column integral of the
    interpolated table over the layers, `gaps` ('zero' or 'hold') saying what an empty layer adds.  The product 'sum' (beside
    'max', 'lowest' or 'echo_top', never with 'source') adds the exact sum of the counting gates' weights per cell and the
    number of gates it skipped (`mean_of` forms the mean): `weight` = {field: (table_v, table_f)} makes the summand of that
    field float32(f(v)) (objects.zr_table(): the rain rate), a field without a table sums its values.  ValueError for what the
    library refuses."""

    def __init__(self, fields, x_edges, y_edges, products=('max',), thresholds=None, height_range=None, plane='radar',
                 z_edges=None, column=None, gaps='zero', weight=None):
        if isinstance(fields, str):
            fields = (fields,)
        fields = tuple(fields)
        if not fields:
            raise ValueError('fields: at least one of %s' % ', '.join(FIELDS))
        for k in fields:
            if k == 'RVEL':
                raise ValueError('RVEL is float64 and is not composed')
            if k not in FIELDS:
                raise ValueError('unknown field %r (one of %s)' % (k, ', '.join(FIELDS)))
        self.fields = tuple(k for k in FIELDS if k in fields)
        self.x_edges = _edges(x_edges, 'x_edges')
        self.y_edges = _edges(y_edges, 'y_edges')
        if isinstance(products, str):
            products = (products,)
        products = tuple(products)
        if not products:
            raise ValueError('products: at least one of %s' % ', '.join(PRODUCTS))
        for q in products:
            if q not in PRODUCTS and q != SOURCE and q != COLUMN and q != SUM:
                raise ValueError('unknown product %r (one of %s)' % (q, ', '.join(PRODUCTS + (SOURCE, COLUMN, SUM))))
        self.products = tuple(q for q in PRODUCTS + (SOURCE, COLUMN, SUM) if q in products)
        if SUM in self.products and not any(q in self.products for q in PRODUCTS):
            raise ValueError("'sum' stands beside 'max', 'lowest' or 'echo_top'")
        if SUM in self.products and SOURCE in self.products:
            raise ValueError("'sum' with 'source': the scratch-and-merge pass carries no sums")
        if SOURCE in self.products and 'max' not in self.products and 'lowest' not in self.products:
            raise ValueError("'source' needs 'max' or 'lowest'")
        if not (callable(plane) or (isinstance(plane, str) and plane in PLANES)):
            raise ValueError('plane: one of %s or a callable f(lats, lons) -> (x, y), got %r' % (', '.join(PLANES), plane))
        self.plane = plane
        self.thresholds = {k: np.zeros(0, dtype=np.float32) for k in self.fields}
        self.thresholds_given = {k: np.zeros(0, dtype=np.float64) for k in self.fields}
        if 'echo_top' in self.products:
            if thresholds is None:
                raise ValueError("'echo_top' needs thresholds")
            if not isinstance(thresholds, dict):
                thresholds = {k: thresholds for k in self.fields}
            for k in thresholds:
                if k not in self.fields:
                    raise ValueError('thresholds of %r, which is not a field of the composite' % (k,))
            for k in self.fields:
                t = np.array(thresholds.get(k, ()), dtype=np.float64).reshape(-1)
                if not 1 <= t.size <= MAX_THRESHOLDS:
                    raise ValueError("'echo_top' needs 1 ... %d thresholds for %s" % (MAX_THRESHOLDS, k))
                if np.any(np.isnan(t)):
                    raise ValueError('a threshold of %s is NaN' % k)
                self.thresholds_given[k] = t
                with np.errstate(over='ignore'):
                    self.thresholds[k] = t.astype(np.float32)
        elif thresholds is not None:
            raise ValueError("thresholds without 'echo_top'")
        self.height_range = None
        if height_range is not None:
            lo, hi = height_range
            lo, hi = _f32(lo), _f32(hi)
            if not lo < hi:
                raise ValueError('height_range: h_lo < h_hi after rounding to float32, got %r' % (height_range,))
            self.height_range = (lo, hi)
            self.height_range_given = (float(height_range[0]), float(height_range[1]))
        # height layers and the column
        self.z_edges = self.z_edges_given = None
        self.column, self.gaps = {}, 'zero'
        if z_edges is not None:
            zg = np.array(z_edges, dtype=np.float64)
            if zg.ndim != 1 or not 2 <= zg.size <= MAX_Z_EDGES:
                raise ValueError('z_edges: 2 ... %d edges in a 1-D sequence' % MAX_Z_EDGES)
            if np.any(np.isnan(zg)):
                raise ValueError('z_edges: an edge is NaN')
            with np.errstate(over='ignore'):
                z = zg.astype(np.float32)
            if not np.all(z[1:] > z[:-1]):
                raise ValueError('z_edges: the edges are not strictly ascending after rounding to float32')
            if self.height_range is not None:
                raise ValueError('z_edges with height_range: the first and last edge are the slab')
            for q in ('lowest', 'echo_top', SOURCE):
                if q in self.products:
                    raise ValueError('z_edges with %r: per layer the composite keeps the maximum and the count alone' % (q,))
            self.z_edges, self.z_edges_given = z, zg
        if COLUMN in self.products:
            if self.z_edges is None:
                raise ValueError("'column' needs z_edges")
            if 'max' not in self.products:
                raise ValueError("'column' needs 'max'")
            if not isinstance(column, dict) or not column:
                raise ValueError("'column' needs column = {field: (table_v, table_f)}")
            if gaps not in GAPS:
                raise ValueError('gaps: one of %s, got %r' % (', '.join(GAPS), gaps))
            self.gaps = gaps
            for k in column:
                if k not in self.fields:
                    raise ValueError('a column table of %r, which is not a field of the composite' % (k,))
            for k in self.fields:
                if k not in column:
                    continue
                tv, tf = column[k]
                tvg = np.array(tv, dtype=np.float64).reshape(-1)
                tf = np.array(tf, dtype=np.float64).reshape(-1)
                if not 2 <= tvg.size <= MAX_TABLE:
                    raise ValueError('the column table of %s: 2 ... %d breakpoints, got %d' % (k, MAX_TABLE, tvg.size))
                if tf.size != tvg.size:
                    raise ValueError('the column table of %s: %d breakpoints and %d values' % (k, tvg.size, tf.size))
                with np.errstate(over='ignore'):
                    tv32 = tvg.astype(np.float32)
                if not (np.all(np.isfinite(tv32)) and np.all(np.isfinite(tf))):
                    raise ValueError('the column table of %s: a breakpoint or a value is NaN or infinite' % k)
                if not np.all(tv32[1:] > tv32[:-1]):
                    raise ValueError('the column table of %s: the breakpoints are not strictly ascending in float32' % k)
                self.column[k] = (tv32, tf)
        else:
            if column is not None:
                raise ValueError("column tables without 'column'")
            if gaps != 'zero':
                raise ValueError("gaps without 'column'")
        # the exact sums
        self.weight = {}
        if weight is not None and SUM not in self.products:
            raise ValueError("weight tables without 'sum'")
        if weight is not None:
            if not isinstance(weight, dict):
                raise ValueError('weight: {field: (table_v, table_f)}, got %r' % (weight,))
            for k in weight:
                if k not in self.fields:
                    raise ValueError('a weight table of %r, which is not a field of the composite' % (k,))
            for k in self.fields:
                if k in weight:
                    self.weight[k] = _table(weight[k], 'the weight table of %s' % k)

    @property
    def n_x(self):
        return len(self.x_edges) - 1

    @property
    def n_y(self):
        return len(self.y_edges) - 1

    @property
    def n_z(self):
        """The number of height layers; 0 without z_edges."""
        return 0 if self.z_edges is None else len(self.z_edges) - 1

    @property
    def mask(self):
        """cpol_composite.fields."""
        return sum(1 << FIELDS.index(k) for k in self.fields)

    @property
    def product_mask(self):
        """cpol_composite.products."""
        return sum(SOURCE_BIT if q == SOURCE else COLUMN_BIT if q == COLUMN else SUM_BIT if q == SUM else 1 << PRODUCTS.index(q)
                   for q in self.products)

    @property
    def gate_plane(self):
        """True where the sweep calls supply per-gate coordinates (CPOL_COMP_PLANE_GATES): every plane but 'radar'."""
        return self.plane != 'radar'

    def planes(self, field):
        """The names of the planes of values[field], in their order."""
        if field not in self.fields:
            raise ValueError('%r is not a field of the composite' % (field,))
        out, src = [], SOURCE in self.products
        if 'max' in self.products:
            out += ['max', 'height_of_max'] + ['source_of_max'] * src
        if 'lowest' in self.products:
            out += ['lowest', 'height_of_lowest'] + ['source_of_lowest'] * src
        return out + ['echo_top_%d' % j for j in range(len(self.thresholds[field]))]

    @property
    def key(self):
        k = (self.fields, self.products, self.x_edges.tobytes(), self.y_edges.tobytes(),
             tuple(self.thresholds[k].tobytes() for k in self.fields),
             None if self.height_range is None else (self.height_range[0].tobytes(), self.height_range[1].tobytes()))
        k = k if self.plane == 'radar' else k + (self.plane,)
        if self.z_edges is not None:          # (a plain spec keeps the key it had)
            k = k + (('z', self.z_edges.tobytes(), self.gaps,
                      tuple((f, tv.tobytes(), tf.tobytes()) for f, (tv, tf) in sorted(self.column.items()))),)
        if SUM in self.products:              # (a spec without 'sum' keeps the key it had)
            k = k + (('w', tuple((f, tv.tobytes(), tf.tobytes()) for f, (tv, tf) in sorted(self.weight.items()))),)
        return k

    def __eq__(self, other):
        return isinstance(other, Composite) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        s = 'Composite(%s, %d x %d cells, products=%s' % ('+'.join(self.fields), self.n_x, self.n_y, '+'.join(self.products))
        if 'echo_top' in self.products:
            s += ', thresholds={%s}' % ', '.join('%s: %s' % (k, [float(t) for t in self.thresholds[k]]) for k in self.fields)
        if self.height_range is not None:
            s += ', height_range=[%g, %g)' % self.height_range
        if self.plane != 'radar':
            s += ', plane=%s' % (self.plane if isinstance(self.plane, str) else getattr(self.plane, '__name__', 'callable'))
        if self.z_edges is not None:
            s += ', %d layers [%g, %g)' % (self.n_z, self.z_edges[0], self.z_edges[-1])
        if self.column:
            s += ', column={%s}, gaps=%s' % (', '.join('%s: %d points' % (k, len(self.column[k][0])) for k in self.fields
                                                         if k in self.column), self.gaps)
        if self.weight:
            s += ', weight={%s}' % ', '.join('%s: %d points' % (k, len(self.weight[k][0])) for k in self.fields if k in self.weight)
        return s + ')'


def grid(half_width, cell):
    """The edges of a uniform axis from -half_width to +half_width (metres) in cells of `cell`: -half_width + cell * j for
    j = 0 ... n with n = round(2 * half_width / cell).  The same array serves east and north."""
    half_width, cell = float(half_width), float(cell)
    if not (cell > 0.0 and half_width > 0.0 and np.isfinite(half_width)):
        raise ValueError('grid: half_width > 0 and cell > 0')
    n = int(round(2.0 * half_width / cell))
    if n < 1 or n + 1 > MAX_EDGES:
        raise ValueError('grid: %d cells; 1 ... %d' % (n, MAX_EDGES - 1))
    return -half_width + cell * np.arange(n + 1, dtype=np.float64)


def from_db(t):
    """dBZ thresholds as linear ones, 10 ** (t / 10): the fields are linear, and the device takes no logarithm."""
    return 10.0 ** (np.asarray(t, dtype=np.float64) / 10.0)


def centers(edges):
    """The midpoints of the cells between `edges`."""
    e = np.asarray(edges, dtype=np.float64)
    return 0.5 * (e[1:] + e[:-1])


def n_blocks(n_rows, rays_per_block=0):
    rpb = int(rays_per_block)
    if rpb < 0 or (rpb and n_rows % rpb):
        raise ValueError('rays_per_block %r does not divide the %d rows of the call' % (rays_per_block, n_rows))
    return n_rows // rpb if rpb else 1


def shape(spec, field, n_rows=1, rays_per_block=0):
    """The shape of values[field] for a call of n_rows rows; with layers the layer axis lies in front of the planes."""
    z = (spec.n_z,) if spec.n_z else ()
    return (n_blocks(n_rows, rays_per_block),) + z + (len(spec.planes(field)), spec.n_y, spec.n_x)


def count_shape(spec, n_rows=1, rays_per_block=0):
    """The shape of the count array; with layers the layer axis lies in front of the fields."""
    z = (spec.n_z,) if spec.n_z else ()
    return (n_blocks(n_rows, rays_per_block),) + z + (len(spec.fields), spec.n_y, spec.n_x)


def column_shape(spec, n_rows=1, rays_per_block=0):
    """The shape of column[field] and of column_layers[field]."""
    return (n_blocks(n_rows, rays_per_block), spec.n_y, spec.n_x)


def sum_shape(spec, n_rows=1, rays_per_block=0):
    """The shape of sum[field] and of sum_skipped[field]: that of count[field]."""
    z = (spec.n_z,) if spec.n_z else ()
    return (n_blocks(n_rows, rays_per_block),) + z + (spec.n_y, spec.n_x)


def state_bytes(spec, blocks):
    """The bytes of the running state of `blocks` blocks (cpol_comp.h: the echo-top states of a field padded to 8 bytes).  With
    'source': the source bytes behind it (one per cell, block and product, each array padded to 8 bytes) and the per-call
    scratch state, as large as the running state without them.  With layers a block holds n_z planes of cells.  With 'sum':
    per field and cell a row of SUM_BINS int64 bins and a uint32 skipped word (the words of a field padded to 8 bytes)."""
    per = int(blocks) * max(spec.n_z, 1) * spec.n_x * spec.n_y
    total = 0
    for k in spec.fields:
        total += per * 8 * (1 + ('max' in spec.products) + ('lowest' in spec.products))
        total += (per * 4 * len(spec.thresholds[k]) + 7) & ~7
        if SUM in spec.products:
            total += per * SUM_BINS * 8 + ((per * 4 + 7) & ~7)
    if SOURCE in spec.products:
        total = 2 * total + len(spec.fields) * (('max' in spec.products) + ('lowest' in spec.products)) * ((per + 7) & ~7)
    return total


def plane_xy(plane, lats, lons, south_pole=None):
    """(x, y), float64, of the delivered float64 `lats` / `lons` of a call on `plane`: 'geographic' -> (lons, lats) in degrees as
    they are; 'model' -> the rotated longitude and latitude through refraction.wgs_to_rotated with `south_pole` (lat, lon: the
    staged model's pole); a callable f(lats, lons) -> (x, y): any projection of the user's.  The
    library takes x and y as they come and computes no trigonometric function itself."""
    lats = np.asarray(lats, dtype=np.float64)
    lons = np.asarray(lons, dtype=np.float64)
    if lats.shape != lons.shape:
        raise ValueError('plane_xy: lats %r and lons %r differ in shape' % (lats.shape, lons.shape))
    if callable(plane):
        x, y = plane(lats, lons)
    elif plane == 'geographic':
        x, y = lons, lats
    elif plane == 'model':
        from .refraction import wgs_to_rotated
        if south_pole is None:
            raise ValueError("plane_xy: the 'model' plane needs south_pole = (lat, lon) of the model's rotated grid")
        y, x = wgs_to_rotated(lats, lons, south_pole[0], south_pole[1])
    else:
        raise ValueError("plane_xy: 'geographic', 'model' or a callable (the radar plane has no per-gate coordinates), got %r" % (plane,))
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if x.shape != lats.shape or y.shape != lats.shape:
        raise ValueError('plane_xy: the plane returned %r and %r for gates of shape %r' % (x.shape, y.shape, lats.shape))
    return x, y


def ray_tables(azimuths):
    """(ray_sin, ray_cos) of azimuths in degrees, float64: what the library is given."""
    az = np.asarray(azimuths, dtype=np.float64).reshape(-1)
    return np.sin(np.deg2rad(az)), np.cos(np.deg2rad(az))


def compose(spec, fields, dist, heights, azimuths, state=None, rays_per_block=0, gate_xy=None, source=0):
    """The rule in NumPy: one call folded into a running state.  fields: {name: float32 [..., n_gates]} for the fields of
    `spec` (leading axes are flattened to rows); dist, heights: float32 [n_rays, n_gates] with n_rays dividing the rows (row r
    takes row r mod n_rays); azimuths: [n_rays] degrees.  `state` (what a former call returned) continues a pass, None begins
    one.  gate_xy = (x, y), float64 [n_rays, n_gates]: the gate plane -- the coordinates are taken as they are, `dist` and
    `azimuths` are not read (both may be None) and a NaN coordinate does not count.  `source` (0 ... 254): this call's number
    for the source_of_* planes of a spec with 'source'.  Returns the state; `finish` decodes it."""
    source = int(source)
    if not 0 <= source < NO_SOURCE:
        raise ValueError('compose: source must lie in 0 ... %d' % (NO_SOURCE - 1))
    with_source = SOURCE in spec.products
    if source and not with_source:
        raise ValueError("compose: a non-zero source without the product 'source'")
    heights = np.asarray(heights)
    if gate_xy is None:
        dist = np.asarray(dist)
        if dist.dtype != np.float32 or heights.dtype != np.float32:
            raise ValueError('compose: dist and heights must be float32')
        ng = dist.shape[-1]
        dist, heights = dist.reshape(-1, ng), heights.reshape(-1, ng)
        n_rays = dist.shape[0]
        rs, rc = ray_tables(azimuths)
        if heights.shape != dist.shape or len(rs) != n_rays:
            raise ValueError('compose: dist and heights are [n_rays, n_gates], azimuths [n_rays]')
        x = dist.astype(np.float64) * rs[:, None]
        y = dist.astype(np.float64) * rc[:, None]
        located = dist == dist
    else:
        x, y = (np.asarray(a) for a in gate_xy)
        if heights.dtype != np.float32 or x.dtype != np.float64 or y.dtype != np.float64:
            raise ValueError('compose: heights must be float32, gate_xy float64')
        ng = heights.shape[-1]
        heights = heights.reshape(-1, ng)
        n_rays = heights.shape[0]
        if x.size != heights.size or y.size != heights.size:
            raise ValueError('compose: gate_xy are [n_rays, n_gates] like heights')
        x, y = x.reshape(n_rays, ng), y.reshape(n_rays, ng)
        located = (x == x) & (y == y)
    ix = np.searchsorted(spec.x_edges, x, side='right') - 1
    iy = np.searchsorted(spec.y_edges, y, side='right') - 1
    geo = located & (heights == heights) & (ix >= 0) & (ix < spec.n_x) & (iy >= 0) & (iy < spec.n_y)
    if spec.height_range is not None:
        geo &= (spec.height_range[0] <= heights) & (heights < spec.height_range[1])
    cell = iy * spec.n_x + ix
    cells = spec.n_x * spec.n_y
    if spec.n_z:
        # the layer of a gate: comparisons in float32 alone; a block holds n_z planes of cells
        iz = np.searchsorted(spec.z_edges, heights, side='right') - 1
        geo &= (iz >= 0) & (iz < spec.n_z)
        cell = iz * cells + cell
        cells = spec.n_z * cells
    cell = np.where(geo, cell, 0)
    kh = key32(heights)
    nb = None
    for k in spec.fields:
        v = np.asarray(fields[k])
        if v.dtype != np.float32:
            raise ValueError('compose: %s must be float32' % k)
        if v.shape[-1] != ng:
            raise ValueError('compose: %s has %d gates, dist %d' % (k, v.shape[-1], ng))
        v = v.reshape(-1, ng)
        rows = v.shape[0]
        if rows % n_rays:
            raise ValueError('compose: %s has %d rows, the geometry %d' % (k, rows, n_rays))
        if nb is None:
            nb = n_blocks(rows, rays_per_block)
            if state is None:
                state = {'spec': spec, 'n_blocks': nb, 'fields': {
                    q: {'max': np.zeros(nb * cells, dtype=_U64), 'lowest': np.full(nb * cells, _LOW_EMPTY, dtype=_U64),
                        'top': np.zeros((len(spec.thresholds[q]), nb * cells), dtype=_U32),
                        'count': np.zeros(nb * cells, dtype=_U64),
                        'source_of_max': np.full(nb * cells, NO_SOURCE, dtype=np.uint8),
                        'source_of_lowest': np.full(nb * cells, NO_SOURCE, dtype=np.uint8)} for q in spec.fields}}
                if SUM in spec.products:
                    state['sum_gates'] = 0
                    for q in spec.fields:
                        state['fields'][q]['sum'] = np.zeros((nb * cells, SUM_BINS), dtype=np.int64)
                        state['fields'][q]['sum_skipped'] = np.zeros(nb * cells, dtype=_U32)
            if state['spec'] != spec or state['n_blocks'] != nb:
                raise ValueError('compose: the spec or the block count differ from the state')
        sel = np.arange(rows) % n_rays
        ok = (v == v) & geo[sel]
        where = (cell[sel] + (np.arange(rows) // (rows // nb))[:, None] * cells)[ok]
        kv = key32(v)[ok].astype(_U64)
        kh_k = kh[sel][ok]
        st = state['fields'][k]
        np.add.at(st['count'], where, _U64(1))
        for q, at, pack, won in (('max', np.maximum.at, (kv << _U64(32)) | kh_k.astype(_U64), np.greater),
                                 ('lowest', np.minimum.at, (kh_k.astype(_U64) << _U64(32)) | kv, np.less)):
            if q not in spec.products:
                continue
            before = st[q].copy() if with_source else None
            at(st[q], where, pack)
            if with_source:
                # the smallest source among the gates of the whole pass that hold the final state: a state this call moved is
                # this call's; one it reached without moving it keeps the smaller number
                byte = st['source_of_' + q]
                byte[won(st[q], before)] = source
                mine = np.zeros(byte.shape, dtype=bool)
                mine[where[pack == st[q][where]]] = True
                byte[mine] = np.minimum(byte[mine], np.uint8(source))
        vv = v[ok]
        if SUM in spec.products:
            # the exact sums: the weight, its split, the bins -- integer additions alone (no bin can wrap: sum_gates)
            from .objects import split, weight_of
            neg, E, M, finite = split(weight_of(vv, spec.weight.get(k)))
            np.add.at(st['sum_skipped'], where[~finite], _U32(1))
            np.add.at(st['sum'], (where[finite], E[finite] >> 3), np.where(neg[finite], -M[finite], M[finite]) << (E[finite] & 7))
        for j, t in enumerate(spec.thresholds[k]):
            above = vv >= t
            np.maximum.at(st['top'][j], where[above], kh_k[above])
    if SUM in spec.products and nb is not None:
        state['sum_gates'] += (rows // nb) * ng
        if state['sum_gates'] > SUM_MAX_GATES:
            raise ValueError("compose: more than 2 ** 32 - 1 gates would fold into one block of the pass ('sum')")
    return state


def finish(state):
    """The state of a pass decoded: {'values': {field: {plane: float32 [n_blocks, n_y, n_x]}}, 'count': {field: uint64
    [n_blocks, n_y, n_x]}}; empty cells NaN."""
    spec, nb = state['spec'], state['n_blocks']
    sh = (nb, spec.n_z, spec.n_y, spec.n_x) if spec.n_z else (nb, spec.n_y, spec.n_x)
    nan = np.float32(np.nan)
    out = {'values': {}, 'count': {}}
    for k in spec.fields:
        st = state['fields'][k]
        planes = {}
        if 'max' in spec.products:
            s = st['max']
            planes['max'] = np.where(s == 0, nan, unkey32((s >> _U64(32)).astype(_U32))).reshape(sh)
            planes['height_of_max'] = np.where(s == 0, nan, unkey32((s & _U64(0xFFFFFFFF)).astype(_U32))).reshape(sh)
            if SOURCE in spec.products:
                planes['source_of_max'] = np.where(s == 0, nan, st['source_of_max'].astype(np.float32)).reshape(sh)
        if 'lowest' in spec.products:
            s = st['lowest']
            planes['lowest'] = np.where(s == _LOW_EMPTY, nan, unkey32((s & _U64(0xFFFFFFFF)).astype(_U32))).reshape(sh)
            planes['height_of_lowest'] = np.where(s == _LOW_EMPTY, nan, unkey32((s >> _U64(32)).astype(_U32))).reshape(sh)
            if SOURCE in spec.products:
                planes['source_of_lowest'] = np.where(s == _LOW_EMPTY, nan, st['source_of_lowest'].astype(np.float32)).reshape(sh)
        for j in range(len(spec.thresholds[k])):
            planes['echo_top_%d' % j] = np.where(st['top'][j] == 0, nan, unkey32(st['top'][j])).reshape(sh)
        out['values'][k] = planes
        out['count'][k] = st['count'].reshape(sh).copy()
    if COLUMN in spec.products:
        out['column'], out['column_layers'] = {}, {}
        for k in spec.fields:
            if k in spec.column:
                out['column'][k], out['column_layers'][k] = column_of(spec, out['values'][k]['max'], field=k)
    if SUM in spec.products:
        from .objects import round_scaled
        out['sum'], out['sum_skipped'] = {}, {}
        for k in spec.fields:
            st = state['fields'][k]
            total = np.full(st['count'].shape, np.nan, dtype=np.float64)
            summed = np.flatnonzero(st['count'] != st['sum_skipped'].astype(_U64))
            for i, row in zip(summed.tolist(), st['sum'][summed].tolist()):
                total[i] = round_scaled(sum(v << (8 * b) for b, v in enumerate(row) if v))
            out['sum'][k] = total.reshape(sh)
            out['sum_skipped'][k] = st['sum_skipped'].reshape(sh).copy()
    return out


def mean_of(res, field):
    """The cell mean of `field` from a result with 'sum' (what `finish`, a composite call or the test hook returns):
    sum / (count - sum_skipped), one float64 division, NaN where the divisor is 0."""
    if 'sum' not in res or field not in res['sum']:
        raise ValueError("mean_of: the result holds no 'sum' of %r" % (field,))
    n = (np.asarray(res['count'][field]).astype(np.int64) - np.asarray(res['sum_skipped'][field]).astype(np.int64)).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(n == 0.0, np.nan, np.asarray(res['sum'][field], dtype=np.float64) / np.where(n == 0.0, 1.0, n))


def column_of(spec, max_planes, field=None):
    """The column integral on its own: (column float64 [n_blocks, n_y, n_x], column_layers uint8 likewise) of the layered `max`
    planes, float32 [n_blocks, n_z, n_y, n_x] (a layer without a counting gate NaN), under the table of `field` (the spec's only
    table when None) and spec.gaps.  Statement by statement what k_comp_column does per cell: the layers ascending, every
    operation one float64 operation."""
    if COLUMN not in spec.products:
        raise ValueError("column_of: the spec has no product 'column'")
    if field is None:
        if len(spec.column) != 1:
            raise ValueError('column_of: name the field whose table is meant (%s)' % ', '.join(spec.column))
        field = next(iter(spec.column))
    if field not in spec.column:
        raise ValueError('column_of: %r has no column table' % (field,))
    tv, tf = spec.column[field]
    n = len(tv)
    m = np.asarray(max_planes)
    if m.dtype != np.float32 or m.ndim != 4 or m.shape[1:] != (spec.n_z, spec.n_y, spec.n_x):
        raise ValueError('column_of: max_planes are float32 [n_blocks, %d, %d, %d]' % (spec.n_z, spec.n_y, spec.n_x))
    ez = spec.z_edges.astype(np.float64)
    tv64 = tv.astype(np.float64)
    sh = (m.shape[0], spec.n_y, spec.n_x)
    have = m == m                                      # (NaN never reaches a state: NaN marks the empty layer)
    any_layer = np.zeros(sh, dtype=bool)
    top = np.full(sh, -1, dtype=np.int64)              # the highest counting layer of the cell
    for l in range(spec.n_z):
        any_layer |= have[:, l]
        top = np.where(have[:, l], l, top)
    total = np.zeros(sh, dtype=np.float64)             # +0.0
    layers = np.zeros(sh, dtype=np.uint8)
    held = np.zeros(sh, dtype=np.float64)
    seen = np.zeros(sh, dtype=bool)                    # a counting layer lies below
    with np.errstate(invalid='ignore', over='ignore'):
        for l in range(spec.n_z):
            v = m[:, l]
            i = np.searchsorted(tv, np.where(have[:, l], v, tv[0]), side='right') - 1
            ii = np.clip(i, 0, n - 2)
            t = (v.astype(np.float64) - tv64[ii]) / (tv64[ii + 1] - tv64[ii])
            d = tf[ii + 1] - tf[ii]
            p = t * d
            f = tf[ii] + p
            f = np.where(i < 0, 0.0, np.where(i >= n - 1, tf[n - 1], f))
            held = np.where(have[:, l], f, held)
            adds = have[:, l]
            if spec.gaps == 'hold':
                adds = adds | (seen & (l < top))
            seen = seen | have[:, l]
            dz = ez[l + 1] - ez[l]
            term = held * dz
            total = np.where(adds, total + term, total)
            layers = layers + adds.astype(np.uint8)
    return np.where(any_layer, total, np.nan), layers


def vil_table(db_min=-10.0, db_cap=56.0, step_db=0.25):
    """The column table of the vertically integrated liquid (Greene and Clark 1972, "Vertically integrated liquid water -- a new
    analysis tool", Mon. Wea. Rev. 100, 548-552): M = 3.44e-6 * Z ** (4 / 7) kg m^-3 with Z in mm^6 m^-3, so that the column
    over layers in metres is kg m^-2.  Returns (float32 Z breakpoints every `step_db` from `db_min` to `db_cap` dBZ, float64
    values): the values are evaluated at the ROUNDED breakpoints with np.power on the host -- the device takes no power.  Below
    db_min a layer adds nothing; at and above db_cap the value stays that of db_cap (the cap against hail)."""
    db_min, db_cap, step_db = float(db_min), float(db_cap), float(step_db)
    if not (step_db > 0.0 and db_cap > db_min):
        raise ValueError('vil_table: db_min < db_cap and step_db > 0')
    n = int(round((db_cap - db_min) / step_db)) + 1
    if not 2 <= n <= MAX_TABLE:
        raise ValueError('vil_table: %d breakpoints; 2 ... %d' % (n, MAX_TABLE))
    db = db_min + step_db * np.arange(n, dtype=np.float64)
    db[-1] = db_cap
    tv = (10.0 ** (db / 10.0)).astype(np.float32)
    return tv, 3.44e-6 * np.power(tv.astype(np.float64), 4.0 / 7.0)


class Maps(object):
    """The composite of ONE sweep call, as RadarOperator._run_rays takes a product ("How a product plugs into a
    sweep call"): this call's gates folded into the lane's running composite.  `phase` and `rays_per_block` may be set anew
    between the calls of a pass; the maps arrive with a finishing call (phase bit 1)."""
    name = 'composite'
    spectrum, model_var = True, None
    refuses = Counts.refuses              # (the two reductions over gates refuse the same calls)

    def __init__(self, spec, keep_gates=False, phase=3, rays_per_block=0, distributed=False):
        # what a composite call refuses before it builds anything.  (Spaceborne geometry is refused by the ray calls
        # themselves: they take ground radars; a spaceborne call, per-ray radar positions, is refused by the library.)
        if not isinstance(spec, Composite):
            raise ValueError('spec: a cosmo_pol_amd.composite.Composite, got %r' % (spec,))
        if distributed:
            raise NotImplementedError('composites with a process group: sharding rays over ranks is not built')
        self.spec, self.gates, self.phase, self.rays_per_block = spec, bool(keep_gates), int(phase), int(rays_per_block)
        self.gate_xy, self.plane_version, self.source = None, 0, 0

    def set_plane(self, gate_xy, plane_version=0, source=0):
        """The call's part of a network composite: gate_xy = (x, y), float64 [n_rays, n_gates] of THIS call's rays on the spec's
        plane (plane_xy of the call's gate coordinates; None on the radar plane), `plane_version` non-zero where the library may
        keep its device copy under that tag, and `source`, the call's number for the source_of_* planes.  May be set anew
        between the calls of a pass, like `phase`."""
        source = int(source)
        if not 0 <= source < NO_SOURCE:
            raise ValueError('source must lie in 0 ... %d, got %d' % (NO_SOURCE - 1, source))
        if source and SOURCE not in self.spec.products:
            raise ValueError("a non-zero source needs the product 'source'")
        if gate_xy is not None and not self.spec.gate_plane:
            raise ValueError("gate_xy goes with a plane other than 'radar'")
        self.gate_xy, self.plane_version, self.source = gate_xy, int(plane_version), source

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        self.n_rows = len(az) * (n_members or 1)
        n_blocks(self.n_rows, self.rays_per_block)            # (ValueError: the library refuses the same)
        xy = self.gate_xy
        if self.spec.gate_plane and xy is None and take is not None:
            raise ValueError('a composite on the plane %r needs the per-gate coordinates of the call (set_plane)' % (self.spec.plane,))
        if xy is not None and any(np.shape(a) != (len(az), n_gates) for a in xy):
            raise ValueError('gate_xy: two arrays [n_rays, n_gates] = %r' % ((len(az), n_gates),))
        # (sine and cosine of the azimuths come from here, the plane coordinates from plane_xy: the library computes neither)
        c, keep = native.Context.composite_struct(self.spec, self.phase, self.rays_per_block, azimuths=None if xy is not None else az,
                                                  gate_xy=xy, source=self.source, plane_version=self.plane_version)
        # (with 'sum' the struct is the wide one: the call points at its member `c`, which shares its memory)
        self.wide = c if SUM in self.spec.products else None
        self.c = c.c if self.wide is not None else c
        keep = keep + [c]
        if self.spec.gate_plane:
            self.c.plane = 1                      # (device outputs: bind_device brings gate_x and gate_y)
        return {'composite': self.c}, keep

    def arrays(self):
        # the maps, in the sweep's own block: they ride the one copy
        if not self.phase & 2:
            return []
        out = ([(k, np.float32, shape(self.spec, k, self.n_rows, self.rays_per_block)) for k in self.spec.fields]
               + [('count', np.uint64, count_shape(self.spec, self.n_rows, self.rays_per_block))])
        if self.spec.column:
            csh = column_shape(self.spec, self.n_rows, self.rays_per_block)
            out += [(('column', k), np.float64, csh) for k in self.spec.fields if k in self.spec.column]
            out += [(('column_layers', k), np.uint8, csh) for k in self.spec.fields if k in self.spec.column]
        if SUM in self.spec.products:
            ssh = sum_shape(self.spec, self.n_rows, self.rays_per_block)
            out += [((SUM, k), np.float64, ssh) for k in self.spec.fields]
            out += [(('sum_skipped', k), np.uint32, ssh) for k in self.spec.fields]
        return out

    def bind(self, path, address):
        if path == 'count':
            self.c.count = address
        elif isinstance(path, tuple):         # ('column' | 'column_layers' | 'sum' | 'sum_skipped', field)
            getattr(self.wide if path[0] in (SUM, 'sum_skipped') else self.c, path[0])[FIELDS.index(path[1])] = address
        else:
            self.c.values[FIELDS.index(path)] = address

    def bind_device(self, entry):         # {'values': {field: device pointer of its float32 planes}, 'count': device pointer}
        entry = dict(entry)               # (a gate plane: 'gate_x', 'gate_y' device pointers of float64 [n_rays, n_gates], any phase)
        for k in ('gate_x', 'gate_y'):
            if k in entry:
                setattr(self.c, k, entry.pop(k))
        for k, ptr in (entry.items() if self.phase & 2 else ()):
            if k not in ('values', 'count', 'column', 'column_layers') + ((SUM, 'sum_skipped') if self.wide is not None else ()):
                raise ValueError("device_outputs['composite']: unknown entry %r" % (k,))
            for f, q in (ptr.items() if k == 'values' else (('count', ptr),) if k == 'count' else (((k, f), q) for f, q in ptr.items())):
                self.bind(f, q)

    def finish(self, w, coords):
        out = self._finish(w)
        if SUM in self.spec.products:
            out[SUM] = {k: w[(SUM, k)] for k in self.spec.fields}
            out['sum_skipped'] = {k: w[('sum_skipped', k)] for k in self.spec.fields}
        return out

    def _finish(self, w):
        spec, cnt = self.spec, w.pop('count')
        if not spec.n_z:
            return {'values': {k: {q: w[k][:, j] for j, q in enumerate(spec.planes(k))} for k in spec.fields},
                    'count': {k: cnt[:, i] for i, k in enumerate(spec.fields)}, 'x_edges': spec.x_edges, 'y_edges': spec.y_edges}
        out = {'values': {k: {q: w[k][:, :, j] for j, q in enumerate(spec.planes(k))} for k in spec.fields},
               'count': {k: cnt[:, :, i] for i, k in enumerate(spec.fields)}, 'x_edges': spec.x_edges, 'y_edges': spec.y_edges,
               'z_edges': spec.z_edges}
        if spec.column:
            out['column'] = {k: w[('column', k)] for k in spec.fields if k in spec.column}
            out['column_layers'] = {k: w[('column_layers', k)] for k in spec.fields if k in spec.column}
        return out

    def join(self, parts, cat):
        """The chunks of an ensemble call: one map per member (rays_per_block set) -> the blocks joined; else the chunks were
        one pass and the last call holds its maps."""
        out = dict(parts[-1])
        if self.rays_per_block:
            out['values'] = {k: {q: cat([w['values'][k][q] for w in parts]) for q in self.spec.planes(k)} for k in self.spec.fields}
            out['count'] = {k: cat([w['count'][k] for w in parts]) for k in self.spec.fields}
            for q in ('column', 'column_layers', SUM, 'sum_skipped'):
                if q in out:
                    out[q] = {k: cat([w[q][k] for w in parts]) for k in out[q]}
        return out
