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
             (n_x + 1) * 4 bytes, at most MAX_SCRATCH_BYTES.

NEIGHBOURHOOD ENSEMBLE PROBABILITIES (cpol_fraction_probabilities; `Probabilities`, `ensemble_sums`; the kernel is k_frac_members,
cosmo_pol_amd/csrc/cpol_frac_prob.inl): what a convective-scale ensemble publishes of its members' maps -- the neighbourhood
ensemble probability (NEP) and the neighbourhood maximum ensemble probability (NMEP; Schwartz and Sobash 2017, Mon. Wea. Rev.
145, 3397-3418), the ensemble FSS of the ensemble-mean fraction (Schwartz et al. 2010; Duc et al. 2013) and a reliability table,
from which the Brier score, the reliability diagram and the ROC follow.
THE RULE
  Inputs are those of cpol_fractions, unchanged.  F[b][t], O[t], NF[b][t][w][y][x] and NO[t][w][y][x] are the binary maps and
  clipped window counts defined there.  M = n_blocks; in an ensemble call a block is a member.
  Per threshold t, radius index w and cell:
    S[t][w][y][x] = sum over b of NF[b][t][w][y][x] (uint32).  NEP is S / (M * window_cells); the division is the host's.
    A[t][w][y][x] = #{ b : NF[b][t][w][y][x] > 0 } (uint32, 0 ... M).  NMEP is A / M.
    OA[t][w][y][x] = NO[t][w][y][x] > 0.
  Both maps are written for EVERY cell of the grid.  The domain only decides which cells are set and which cells are summed.
  Sums over the cells of the domain, uint64:
    prob_sums[t][w][3] = (diff2, forecast2, observed2): diff2 = sum (S - M * NO)^2, forecast2 = sum S^2, observed2 = M^2 * sum
    NO^2.  neighbourhood.fss applied to these three gives the ensemble FSS unchanged.  With M == 1 they equal block 0's row of
    `sums`.
    reliability[t][w][k][o], k = 0 ... M, o = 0 | 1: the number of domain cells with A == k and OA == o.  At radius 0 this is the
    classic table "k of M members exceed, observed yes or no".  At larger radii it is the NMEP against the neighbourhood-maximum
    observation.  Every [t][w] slice sums to n_domain.
  Limits are conditions, not measurements.
    1 <= n_blocks <= MAX_PROB_BLOCKS (256); it bounds `reliability` and the kernel's LDS table.
    NO OVERFLOW, checked before anything is queued (`overflows`).  Let c = min(2 * r_max + 1, n_y) * min(2 * r_max + 1, n_x).
    The call is refused unless M * c < 2^32 and n_y * n_x * (M * c)^2 < 2^64.  |S - M * NO| <= M * c, so the bound covers all
    three sums.
  The result depends neither on the order of the blocks nor on how the work is cut.
  NOT BUILT: Probabilities over an objects.Objects in Python (the C structs may stand side by side); a member list cut into
  several chunks (the sums are not additive over chunks)."""
import numpy as np

from .composite import FIELDS, Composite, Maps

MAX_THRESHOLDS = 4
MAX_RADII = 8
MAX_RADIUS = 1023
MAX_SCRATCH_BYTES = 1 << 30
MAX_PROB_BLOCKS = 256

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


# ---------------------------------------------------------------------------------------- neighbourhood ensemble probabilities
class Probabilities(object):
    """A `Fractions` whose scored call also reduces the neighbourhood ensemble probabilities of its blocks (the rule at the head of
    this module): the sums of the ensemble FSS and the reliability table always, the S maps (`maps`: NEP = S / (M *
    window_cells)) and the A maps (`any_maps`: NMEP = A / M) when asked for.  Accepted wherever a Fractions is.  ValueError over
    an objects.Objects: that combination is not built in Python."""

    def __init__(self, fractions, maps=False, any_maps=False):
        if not isinstance(fractions, Fractions):
            from .objects import Objects
            if isinstance(fractions, Objects):
                raise ValueError('Probabilities over an objects.Objects is not built in Python: wrap the Fractions, and ask for '
                                 'the object cells in a call of their own')
            raise ValueError('fractions: a cosmo_pol_amd.neighbourhood.Fractions, got %r' % (fractions,))
        self.fractions, self.maps, self.any_maps = fractions, bool(maps), bool(any_maps)

    composite = property(lambda self: self.fractions.composite)
    thresholds = property(lambda self: self.fractions.thresholds)
    thresholds_given = property(lambda self: self.fractions.thresholds_given)
    radii = property(lambda self: self.fractions.radii)
    n_x = property(lambda self: self.fractions.n_x)
    n_y = property(lambda self: self.fractions.n_y)

    @property
    def key(self):
        return (self.fractions.key, self.maps, self.any_maps)

    def __eq__(self, other):
        return isinstance(other, Probabilities) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return 'Probabilities(%r, maps=%r, any_maps=%r)' % (self.fractions, self.maps, self.any_maps)


def _fractions_of(spec):
    return spec.fractions if isinstance(spec, Probabilities) else spec


def overflows(n_x, n_y, n_blocks, r_max):
    """The NO OVERFLOW condition of the rule in Python integers: True where a call is refused."""
    side = 2 * int(r_max) + 1
    mc = int(n_blocks) * min(side, int(n_y)) * min(side, int(n_x))
    return mc >= 1 << 32 or int(n_y) * int(n_x) * mc * mc >= 1 << 64


def ensemble_result(spec, n_blocks, prob_sums, reliability, member_sum=None, member_any=None):
    """The output arrays named: {'diff2' | 'forecast2' | 'observed2': uint64 [n_thr, n_radii], 'reliability': uint64 [n_thr,
    n_radii, M + 1, 2], 'member_sum' | 'member_any': uint32 [n_thr, n_radii, n_y, n_x] when given, 'n_blocks', 'thresholds',
    'radii'}."""
    out = {'diff2': prob_sums[..., 0], 'forecast2': prob_sums[..., 1], 'observed2': prob_sums[..., 2], 'reliability': reliability,
           'n_blocks': int(n_blocks), 'thresholds': spec.thresholds, 'radii': spec.radii}
    if member_sum is not None:
        out['member_sum'] = member_sum
    if member_any is not None:
        out['member_any'] = member_any
    return out


def ensemble_sums(spec, plane_maps, observed, domain=None):
    """The rule of the neighbourhood ensemble probabilities in NumPy.  spec: a Fractions or a Probabilities; plane_maps: float32
    [n_blocks, n_y, n_x] (or [n_y, n_x]: one block); observed, domain: see check_maps.  Returns what `ensemble_result` describes,
    always with both maps.  ValueError for more than MAX_PROB_BLOCKS blocks and where the sums could overflow."""
    spec = _fractions_of(spec)
    m = np.asarray(plane_maps)
    if m.dtype != np.float32:
        raise ValueError('plane_maps must be float32, got %s' % m.dtype)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (spec.n_y, spec.n_x) or m.shape[0] < 1:
        raise ValueError('plane_maps: [n_blocks, %d, %d], got %r' % (spec.n_y, spec.n_x, m.shape))
    M = m.shape[0]
    if M > MAX_PROB_BLOCKS:
        raise ValueError('probabilities: at most %d blocks, got %d' % (MAX_PROB_BLOCKS, M))
    if overflows(spec.n_x, spec.n_y, M, spec.radii[-1]):
        raise ValueError('probabilities: the sums of %d blocks with radius %d could overflow' % (M, spec.radii[-1]))
    o, domain = check_maps(spec, observed, domain)
    dom = np.ones(o.shape, dtype=bool) if domain is None else domain != 0
    thr = spec.thresholds[:, None, None]
    nt, nr = len(spec.thresholds), len(spec.radii)
    S = np.zeros((nt, nr) + o.shape, dtype=_I64)
    A = np.zeros((nt, nr) + o.shape, dtype=_I64)
    with np.errstate(invalid='ignore'):
        O = dom & (o == o) & (o[None] >= thr)                               # [n_thr, n_y, n_x]
        for b in range(M):                                                  # (a block at a time: 256 blocks need no 256 tables)
            NF = _window_counts(dom & (m[b] == m[b]) & (m[b][None] >= thr), spec.radii)
            S += NF
            A += NF > 0
    NO = _window_counts(O, spec.radii)                                      # [n_thr, n_radii, n_y, n_x]
    # (uint64 from the squares on: the condition above bounds every term below 2^64 and every sum too, not below 2^63)
    s = np.empty((nt, nr, 3), dtype=_U64)
    Sd, NOd = S[..., dom], NO[..., dom] * M
    for k, v in enumerate((np.abs(Sd - NOd), Sd, NOd)):
        v = v.astype(_U64)
        s[..., k] = (v * v).sum(axis=-1, dtype=_U64)
    rel = np.zeros((nt, nr, M + 1, 2), dtype=_U64)
    Ad, OAd = A[..., dom], (NO > 0)[..., dom]
    for t in range(nt):
        for w in range(nr):
            rel[t, w] = np.bincount(Ad[t, w] * 2 + OAd[t, w], minlength=2 * (M + 1)).reshape(M + 1, 2).astype(_U64)
    return ensemble_result(spec, M, s, rel, S.astype(np.uint32), A.astype(np.uint32))


def window_cells(spec, domain=None):
    """int64 [n_radii, n_y, n_x]: the cells of each clipped window -- what a set count NF is a fraction of.  With `domain` (uint8 or
    bool [n_y, n_x]) the cells of the domain inside it: outside the domain nothing is set."""
    spec = _fractions_of(spec)
    inside = np.ones((spec.n_y, spec.n_x), dtype=bool) if domain is None else np.asarray(domain).reshape(spec.n_y, spec.n_x) != 0
    return _window_counts(inside, spec.radii)


def nep(res, cells):
    """The neighbourhood ensemble probability, float64 [n_thr, n_radii, n_y, n_x]: member_sum / (n_blocks * cells), `cells` from
    window_cells; NaN where a window holds no cell of the domain.  ValueError when the S maps were not asked for."""
    if 'member_sum' not in res:
        raise ValueError("nep: needs the S maps (Probabilities(maps=True)), the result has no 'member_sum'")
    with np.errstate(invalid='ignore', divide='ignore'):
        return res['member_sum'].astype(np.float64) / (float(res['n_blocks']) * np.asarray(cells, dtype=np.float64))


def nmep(res):
    """The neighbourhood maximum ensemble probability, float64 [n_thr, n_radii, n_y, n_x]: member_any / n_blocks.  ValueError
    when the A maps were not asked for."""
    if 'member_any' not in res:
        raise ValueError("nmep: needs the A maps (Probabilities(any_maps=True)), the result has no 'member_any'")
    return res['member_any'].astype(np.float64) / float(res['n_blocks'])


def _table(res):
    n = res['reliability'].astype(np.float64)                               # [n_thr, n_radii, M + 1, 2]
    return n, np.arange(n.shape[-2], dtype=np.float64) / float(n.shape[-2] - 1)


def brier(res):
    """The Brier score of the forecast probability k / M against the observed event, float64 [n_thr, n_radii], from the
    reliability table: sum_k (n[k, 0] (k / M)^2 + n[k, 1] (k / M - 1)^2) / n_domain; NaN for an empty domain."""
    n, p = _table(res)
    with np.errstate(invalid='ignore', divide='ignore'):
        return (n[..., 0] * p ** 2 + n[..., 1] * (p - 1.0) ** 2).sum(axis=-1) / n.sum(axis=(-2, -1))


def reliability_curve(res):
    """The reliability diagram: {'probability': k / M, float64 [M + 1]; 'observed_frequency': n[k, 1] / (n[k, 0] + n[k, 1]),
    float64 [n_thr, n_radii, M + 1], NaN where no cell forecast k / M; 'count': uint64 [n_thr, n_radii, M + 1]}."""
    n, p = _table(res)
    with np.errstate(invalid='ignore', divide='ignore'):
        return {'probability': p, 'observed_frequency': n[..., 1] / n.sum(axis=-1), 'count': res['reliability'].sum(axis=-1)}


def roc(res):
    """The relative operating characteristic of the decision "at least k members", k = 0 ... M + 1: {'pod': hits / observed yes,
    'pofd': false alarms / observed no, float64 [n_thr, n_radii, M + 2], from (1, 1) at k = 0 down to (0, 0); NaN where the
    event was never (always) observed; 'area': the trapezoid area under pod over pofd, float64 [n_thr, n_radii]}."""
    n, _ = _table(res)
    tail = np.concatenate([np.cumsum(n[..., ::-1, :], axis=-2)[..., ::-1, :], np.zeros(n.shape[:-2] + (1, 2))], axis=-2)
    with np.errstate(invalid='ignore', divide='ignore'):
        pofd, pod = tail[..., 0] / tail[..., :1, 0], tail[..., 1] / tail[..., :1, 1]
    area = -((pofd[..., 1:] - pofd[..., :-1]) * (pod[..., 1:] + pod[..., :-1]) / 2.0).sum(axis=-1)
    return {'pod': pod, 'pofd': pofd, 'area': area}


class EnsembleScores(Scores):
    """A scored composite of ONE sweep call WITH the neighbourhood ensemble probabilities of its blocks: a `Scores`, and behind a
    finishing call the cpol_fractions_ensemble around its cpol_fractions, which points to the cpol_fraction_probabilities.  The new slots are handled the way `sums`
    and `totals` are."""
    one_chunk = 'the sums are not additive over chunks'     # (_ensemble_reduced: needs the members in one chunk)
    _OWN = ('prob_sums', 'reliability', 'member_sum', 'member_any')

    def __init__(self, spec, observed=None, domain=None, keep_gates=False, phase=3, rays_per_block=0, distributed=False):
        if not isinstance(spec, Probabilities):
            raise ValueError('spec: a cosmo_pol_amd.neighbourhood.Probabilities, got %r' % (spec,))
        Scores.__init__(self, spec.fractions, observed, domain, keep_gates, phase, rays_per_block, distributed)
        self.prob, self.q = spec, None

    def _wanted(self):
        return self._OWN[:2] + (('member_sum',) if self.prob.maps else ()) + (('member_any',) if self.prob.any_maps else ())

    def attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take):
        structs, keep = Scores.attach(self, native, az, n_gates, n_members, doppler, spectrum, staged_vars, take)
        self.q = None
        if self.f is None:                        # (no cpol_fractions in this call: nothing to hang on)
            return structs, keep
        if self.n_blocks > MAX_PROB_BLOCKS:
            raise ValueError('probabilities: at most %d blocks, got %d' % (MAX_PROB_BLOCKS, self.n_blocks))
        if overflows(self.spec.n_x, self.spec.n_y, self.n_blocks, self.spec.radii[-1]):
            raise ValueError('probabilities: the sums of %d blocks with radius %d could overflow' % (self.n_blocks, self.spec.radii[-1]))
        # the cpol_fractions becomes the first member of a cpol_fractions_ensemble; self.f is from here on the copy inside it
        self.f, self.q, qkeep = native.Context.probabilities_struct(self.f)
        return dict(structs, fractions=self.f), keep + qkeep

    def arrays(self):
        out = Scores.arrays(self)
        if self.phase & 2:
            spec, nt, nr = self.spec, len(self.spec.thresholds), len(self.spec.radii)
            shapes = {'prob_sums': (np.uint64, (nt, nr, 3)), 'reliability': (np.uint64, (nt, nr, self.n_blocks + 1, 2)),
                      'member_sum': (np.uint32, (nt, nr, spec.n_y, spec.n_x)), 'member_any': (np.uint32, (nt, nr, spec.n_y, spec.n_x))}
            out = out + [(k,) + shapes[k] for k in self._wanted()]
        return out

    def bind(self, path, address):
        if path in self._OWN:
            setattr(self.q, path, address)
        else:
            Scores.bind(self, path, address)

    def bind_device(self, entry):
        # the scores' entries and 'prob_sums' | 'reliability' | 'member_sum' | 'member_any': device pointers
        rest = {}
        for k, ptr in entry.items():
            if k in self._OWN and self.phase & 2 and k in self._wanted():
                self.bind(k, ptr)
            else:
                rest[k] = ptr
        Scores.bind_device(self, rest)

    def finish(self, w, coords):
        own = {k: w.pop(k) for k in self._wanted()}
        out = Scores.finish(self, w, coords)
        out['probabilities'] = ensemble_result(self.spec, self.n_blocks, own['prob_sums'], own['reliability'],
                                               own.get('member_sum'), own.get('member_any'))
        return out

    def join(self, parts, cat):
        if len(parts) > 1:
            raise ValueError('probabilities: needs the members in one chunk (%s)' % self.one_chunk)
        return Scores.join(self, parts, cat)
