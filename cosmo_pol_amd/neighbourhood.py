"""Neighbourhood verification (cpol_fractions): the sums of the fractions skill score (FSS; Roberts and Lean 2008, Mon. Wea.
Rev. 136, 78-97) of one finished plane of a composite against an observed map on the same grid, per block, threshold and
neighbourhood size, reduced on the device.  This module states the rule in NumPy (`sums`); include/cosmo_pol_amd.h states the
same text, and the GPU tests compare the kernels (cosmo_pol_amd/csrc/cpol_frac.inl) with it exactly: every intermediate is a
count of integers.

THE RULE
  Input      one finished plane of one field of a composite, float32 m[n_blocks, n_y, n_x]: any name out of
             spec.planes(field) ('max' by default), exactly as the composite's finish leaves it, empty cells NaN.  `observed`,
             float32 o[n_y, n_x] on the same grid in the field's own linear units, NaN = no echo or no data.  Optional `domain`,
             uint8 [n_y, n_x], non-zero = the cell belongs to the verification domain; without it every cell does.
  Thresholds 1 ... MAX_THRESHOLDS values, each rounded once to float32, not NaN; -inf and +inf are allowed.
  Radii      1 ... MAX_RADII integers r, strictly ascending, 0 <= r <= MAX_RADIUS; the window is (2r + 1) x (2r + 1) cells.
  Binary     F[b, t] = domain & (m == m) & (m >= thr[t]);  O[t] = domain & (o == o) & (o >= thr[t]): float32 comparisons alone.
  Counts     NF[b, t, w][y, x] = the number of set cells (y', x') of F[b, t] with |y' - y| <= r_w and |x' - x| <= r_w INSIDE the
             grid: the window is clipped at the border, nothing is set outside the grid.  NO[t, w] likewise of O[t].
  Sums       over the cells of the domain, uint64: diff2 = sum (NF - NO)^2, forecast2 = sum NF^2, observed2 = sum NO^2 per
             (b, t, w); n_forecast = sum F, n_observed = sum O, n_domain = sum domain per (b, t).
  Overflow   none is possible: a grid has at most 1023 x 1023 < 2^20 cells (composite.MAX_EDGES), so a count is < 2^20, a
             square < 2^40 and a sum over the cells < 2^60.
  Outputs    sums uint64 [n_blocks][n_thr][n_radii][3] (diff2, forecast2, observed2); totals uint64 [n_blocks][n_thr][3]
             (n_forecast, n_observed, n_domain).  `result` names them.
  Score      FSS = 1 - diff2 / (forecast2 + observed2) in float64 on the host (`fss`), NaN where both maps are empty.
  Limits     the summed-area tables of all blocks and thresholds and of the observation, (n_blocks + 1) * n_thr * (n_y + 1) *
             (n_x + 1) * 4 bytes, at most MAX_SCRATCH_BYTES."""
import numpy as np

from .composite import FIELDS, Composite, Maps

MAX_THRESHOLDS = 4
MAX_RADII = 8
MAX_RADIUS = 1023
MAX_SCRATCH_BYTES = 1 << 30

_U64, _I64 = np.uint64, np.int64


class Fractions(object):
    """What a scoring call reduces: the finished plane `plane` (a name out of composite_spec.planes(field)) of `field` of the
    composite `composite_spec` (a composite.Composite), thresholded at `thresholds` (1 ... 4, the field's own linear units;
    composite.from_db makes them from dBZ) and counted in square neighbourhoods of `radii` cells (1 ... 8 integers, strictly
    ascending, 0 ... 1023).  ValueError for what the library refuses."""

    def __init__(self, composite_spec, field, thresholds, radii, plane='max'):
        if not isinstance(composite_spec, Composite):
            raise ValueError('composite_spec: a cosmo_pol_amd.composite.Composite, got %r' % (composite_spec,))
        if composite_spec.n_z:
            raise ValueError('a composite with height layers is not scored: its planes carry a layer axis, and the column is no plane')
        if field == 'RVEL':
            raise ValueError('RVEL is float64 and is not composed')
        if field not in composite_spec.fields:
            raise ValueError('%r is not a field of the composite (%s)' % (field, ', '.join(composite_spec.fields)))
        planes = composite_spec.planes(field)
        if plane not in planes:
            raise ValueError('%r is not a plane of %s (%s)' % (plane, field, ', '.join(planes)))
        if str(plane).startswith('source_of_'):
            raise ValueError('%r names the radar of a cell and has no units to threshold: not a plane to score' % (plane,))
        t = np.array(thresholds, dtype=np.float64).reshape(-1)
        if not 1 <= t.size <= MAX_THRESHOLDS:
            raise ValueError('thresholds: 1 ... %d values, got %d' % (MAX_THRESHOLDS, t.size))
        if np.any(np.isnan(t)):
            raise ValueError('a threshold is NaN')
        r = np.array(radii).reshape(-1)
        if not 1 <= r.size <= MAX_RADII:
            raise ValueError('radii: 1 ... %d values, got %d' % (MAX_RADII, r.size))
        if r.dtype.kind not in 'iu':
            if r.dtype.kind != 'f' or not np.all(np.isfinite(r)) or np.any(r != np.round(r)):
                raise ValueError('radii: integers (cells), got %r' % (radii,))
        if np.any(r < 0) or np.any(r > MAX_RADIUS):
            raise ValueError('a radius lies outside 0 ... %d' % MAX_RADIUS)
        r = r.astype(np.int32)
        if np.any(r[1:] <= r[:-1]):
            raise ValueError('the radii are not strictly ascending')
        self.composite, self.field, self.plane = composite_spec, field, plane
        self.plane_index = planes.index(plane)
        self.thresholds_given = t
        with np.errstate(over='ignore'):
            self.thresholds = t.astype(np.float32)
        self.radii = r

    @property
    def n_x(self):
        return self.composite.n_x

    @property
    def n_y(self):
        return self.composite.n_y

    @property
    def key(self):
        return (self.composite.key, self.field, self.plane, self.thresholds.tobytes(), self.radii.tobytes())

    def __eq__(self, other):
        return isinstance(other, Fractions) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return 'Fractions(%s %s of %r, thresholds=%s, radii=%s)' % (self.field, self.plane, self.composite,
                                                                   [float(t) for t in self.thresholds], [int(r) for r in self.radii])


def scratch_bytes(spec, blocks):
    """The bytes of the summed-area tables of `blocks` blocks and the observation (cpol_frac.h)."""
    return (int(blocks) + 1) * len(spec.thresholds) * (spec.n_y + 1) * (spec.n_x + 1) * 4


def check_maps(spec, observed, domain=None):
    """`observed` and `domain` as the library takes them: float32 and uint8 [n_y, n_x], C-contiguous.  ValueError for a wrong
    shape or dtype (nothing is converted: a float64 map would be thresholded differently)."""
    sh = (spec.n_y, spec.n_x)
    observed = np.asarray(observed)
    if observed.dtype != np.float32 or observed.shape != sh:
        raise ValueError('observed: float32 %r, got %s %r' % (sh, observed.dtype, observed.shape))
    if domain is not None:
        domain = np.asarray(domain)
        if domain.dtype == np.bool_:
            domain = domain.view(np.uint8)
        if domain.dtype != np.uint8 or domain.shape != sh:
            raise ValueError('domain: uint8 (or bool) %r, got %s %r' % (sh, domain.dtype, domain.shape))
        domain = np.ascontiguousarray(domain)
    return np.ascontiguousarray(observed), domain


def _window_counts(binary, radii):
    """int64 [..., n_radii, n_y, n_x]: the set cells of `binary` [..., n_y, n_x] in each clipped window, from a summed-area table
    (two cumsums) and four look-ups per cell."""
    n_y, n_x = binary.shape[-2:]
    table = np.zeros(binary.shape[:-2] + (n_y + 1, n_x + 1), dtype=_I64)
    table[..., 1:, 1:] = binary.astype(_I64).cumsum(axis=-2).cumsum(axis=-1)
    y, x = np.arange(n_y), np.arange(n_x)
    out = np.empty(binary.shape[:-2] + (len(radii), n_y, n_x), dtype=_I64)
    for w, r in enumerate(radii):
        y0, y1 = np.maximum(y - r, 0)[:, None], (np.minimum(y + r, n_y - 1) + 1)[:, None]
        x0, x1 = np.maximum(x - r, 0)[None, :], (np.minimum(x + r, n_x - 1) + 1)[None, :]
        out[..., w, :, :] = table[..., y1, x1] - table[..., y0, x1] - table[..., y1, x0] + table[..., y0, x0]
    return out


def result(spec, sums_array, totals_array):
    """The two output arrays named: {'diff2' | 'forecast2' | 'observed2': uint64 [n_blocks, n_thr, n_radii], 'n_forecast' |
    'n_observed' | 'n_domain': uint64 [n_blocks, n_thr], 'thresholds', 'radii'}."""
    return {'diff2': sums_array[..., 0], 'forecast2': sums_array[..., 1], 'observed2': sums_array[..., 2],
            'n_forecast': totals_array[..., 0], 'n_observed': totals_array[..., 1], 'n_domain': totals_array[..., 2],
            'thresholds': spec.thresholds, 'radii': spec.radii}


def sums(spec, plane_maps, observed, domain=None):
    """The rule in NumPy.  plane_maps: float32 [n_blocks, n_y, n_x] (or [n_y, n_x]: one block), the plane `spec.plane` of
    `spec.field` as a composite's finish returns it; observed, domain: see check_maps.  Returns what `result` describes."""
    m = np.asarray(plane_maps)
    if m.dtype != np.float32:
        raise ValueError('plane_maps must be float32, got %s' % m.dtype)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (spec.n_y, spec.n_x) or m.shape[0] < 1:
        raise ValueError('plane_maps: [n_blocks, %d, %d], got %r' % (spec.n_y, spec.n_x, m.shape))
    o, domain = check_maps(spec, observed, domain)
    dom = np.ones(o.shape, dtype=bool) if domain is None else domain != 0
    thr = spec.thresholds[:, None, None]
    with np.errstate(invalid='ignore'):
        F = dom & (m == m)[:, None] & (m[:, None] >= thr)                   # [n_blocks, n_thr, n_y, n_x]
        O = dom & (o == o) & (o[None] >= thr)                               # [n_thr, n_y, n_x]
    NF = _window_counts(F, spec.radii)                                      # [n_blocks, n_thr, n_radii, n_y, n_x]
    NO = _window_counts(O, spec.radii)[None]
    s = np.empty(F.shape[:2] + (len(spec.radii), 3), dtype=_U64)
    s[..., 0] = ((NF - NO) ** 2)[..., dom].sum(axis=-1).astype(_U64)
    s[..., 1] = (NF ** 2)[..., dom].sum(axis=-1).astype(_U64)
    s[..., 2] = np.broadcast_to((NO ** 2)[..., dom].sum(axis=-1), s.shape[:-1]).astype(_U64)
    t = np.empty(F.shape[:2] + (3,), dtype=_U64)
    t[..., 0] = F.sum(axis=(-2, -1), dtype=_I64).astype(_U64)
    t[..., 1] = O.sum(axis=(-2, -1), dtype=_I64).astype(_U64)[None]
    t[..., 2] = _U64(int(dom.sum()))
    return result(spec, s, t)


def fss(res):
    """The fractions skill score, float64 [n_blocks, n_thr, n_radii]: 1 - diff2 / (forecast2 + observed2); NaN where
    forecast2 + observed2 == 0 (neither map exceeds the threshold anywhere in the domain)."""
    den = res['forecast2'].astype(np.float64) + res['observed2'].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den == 0.0, np.nan, 1.0 - res['diff2'].astype(np.float64) / den)


def bias(res):
    """The frequency bias n_forecast / n_observed, float64 [n_blocks, n_thr] (inf or NaN where nothing was observed)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return res['n_forecast'].astype(np.float64) / res['n_observed'].astype(np.float64)


def contingency(res):
    """{'hits', 'misses', 'false_alarms', 'correct_negatives': uint64 [n_blocks, n_thr]} from the radius-0 row, where the
    counts are the binary maps themselves: forecast2 = n_forecast, observed2 = n_observed and diff2 counts the cells where the
    two differ, so hits = (forecast2 + observed2 - diff2) / 2.  ValueError when radius 0 was not requested."""
    radii = [int(r) for r in res['radii']]
    if 0 not in radii:
        raise ValueError('contingency: needs the radius-0 row, the radii are %r' % (radii,))
    w = radii.index(0)
    f2, o2, d2 = (res[k][..., w].astype(_I64) for k in ('forecast2', 'observed2', 'diff2'))
    hits = (f2 + o2 - d2) // 2
    misses, false_alarms = o2 - hits, f2 - hits
    negatives = res['n_domain'].astype(_I64) - hits - misses - false_alarms
    return {'hits': hits.astype(_U64), 'misses': misses.astype(_U64), 'false_alarms': false_alarms.astype(_U64),
            'correct_negatives': negatives.astype(_U64)}


class Scores(object):
    """A composite of ONE sweep call WITH its scores, as RadarOperator._run_rays takes a product ("How a product plugs
    into a sweep call"): a composite.Maps, and behind a finishing call (phase bit 1) the cpol_fractions of its finished plane.
    It answers for both struct slots; `phase` and `rays_per_block` are the Maps' and may be set anew between the calls of a pass.
    `observed`, `domain`: as check_maps returns them (None with device outputs: device_outputs['composite'] carries them)."""
    name = 'composite'
    spectrum, model_var = True, None
    refuses = Maps.refuses

    def __init__(self, spec, observed=None, domain=None, keep_gates=False, phase=3, rays_per_block=0, distributed=False):
        if not isinstance(spec, Fractions):
            raise ValueError('spec: a cosmo_pol_amd.neighbourhood.Fractions, got %r' % (spec,))
        self.maps = Maps(spec.composite, keep_gates, phase, rays_per_block, distributed)     # (the refusals are those of Maps)
        self.spec, self.gates, self.observed, self.domain = spec, self.maps.gates, observed, domain
        self.f = None

    def set_plane(self, gate_xy, plane_version=0, source=0):
        self.maps.set_plane(gate_xy, plane_version, source)

    phase = property(lambda self: self.maps.phase, lambda self, v: setattr(self.maps, 'phase', int(v)))
    rays_per_block = property(lambda self: self.maps.rays_per_block, lambda self, v: setattr(self.maps, 'rays_per_block', int(v)))

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        structs, keep = self.maps.attach(native, az, n_gates, n_members, doppler, spectrum, staged_vars, take)
        self.f = None
        if not self.phase & 2:                    # (the maps do not exist yet: the library refuses the struct)
            return structs, keep
        spec = self.spec
        self.n_blocks = self.maps.n_rows // self.rays_per_block if self.rays_per_block else 1
        if scratch_bytes(spec, self.n_blocks) > MAX_SCRATCH_BYTES:
            raise ValueError('fractions: the summed-area tables of %d blocks need more than 1 GiB' % self.n_blocks)
        self.f, fkeep = native.Context.fractions_struct(spec)
        keep = keep + fkeep
        if take is not None:
            # the observed map and the domain in a page-locked block of their own, which the device reads in place.  (A clean
            # block: no writer is named, so none whose last copy may still be in flight -- the host writes it now.)
            if self.observed is None:
                raise ValueError('fractions: a finishing call needs the observed map')
            block = [('observed', np.float32, (spec.n_y, spec.n_x))]
            if self.domain is not None:
                block.append(('domain', np.uint8, (spec.n_y, spec.n_x)))
            views, addresses = take(block)
            for (k, _, _), v, a in zip(block, views, addresses):
                v[...] = getattr(self, k)
                setattr(self.f, k, a)
            keep = keep + views                   # (the block: the kernels read it until this call is done)
        return dict(structs, fractions=self.f), keep

    def arrays(self):
        # the maps, then the scores, in the sweep's own block: they ride the one copy
        out = self.maps.arrays()
        if self.phase & 2:
            nt, nr = len(self.spec.thresholds), len(self.spec.radii)
            out = out + [('sums', np.uint64, (self.n_blocks, nt, nr, 3)), ('totals', np.uint64, (self.n_blocks, nt, 3))]
        return out

    def bind(self, path, address):
        if path in ('sums', 'totals', 'observed', 'domain'):
            setattr(self.f, path, address)
        else:
            self.maps.bind(path, address)

    def bind_device(self, entry):
        # the composite's entries and 'observed' | 'domain' | 'sums' | 'totals': device pointers
        rest = {}
        for k, ptr in (entry.items() if self.phase & 2 else ()):
            if k in ('sums', 'totals', 'observed', 'domain'):
                self.bind(k, ptr)
            else:
                rest[k] = ptr
        self.maps.bind_device(rest)

    def finish(self, w, coords):
        s, t = w.pop('sums'), w.pop('totals')
        out = self.maps.finish(w, coords)
        out['fractions'] = result(self.spec, s, t)
        return out

    def join(self, parts, cat):
        """The chunks of an ensemble call: a block per member -> the blocks joined; else the last call holds the pass."""
        out = self.maps.join(parts, cat)
        if self.rays_per_block:
            fr = [w['fractions'] for w in parts]
            out['fractions'] = dict(fr[-1], **{k: cat([q[k] for q in fr]) for k in
                                               ('diff2', 'forecast2', 'observed2', 'n_forecast', 'n_observed', 'n_domain')})
        return out
