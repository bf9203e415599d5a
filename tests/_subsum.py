"""Inputs and a plain restatement for the sub-beam sums (k_subbeam_sum_gather / _lds / _scalar, k_subbeam_sum_team<W, CHAIN> and
the sub-beam loops of k_final, cosmo_pol_amd/csrc/cpol_final.inl).

Every form has to reproduce nansum([float32 sum, float64 term]) stored back as float32, sub-beam after sub-beam.  What decides
whether a form does is the NUMBER of sub-beams (chunks of 64 validity bits, rounds of W sub-beams per team, groups of 7 and of
2 in k_final), the TILE a wavefront's 64 lanes cover (16 rays x 4 gates down to 1 x 64) and WHICH sub-beams hold a species
in which lanes.  Here are
  * make_columns(case): the dict RadarOperator.simulate_columns takes, for the 1-moment configuration with melting and ice
    crystals (R, S, G, mS, mG, I: the species of the radial case c4_7x7) with the melting fields GIVEN -- presence is then
    exactly what the builder says: a species is present at (ray, sub-beam, gate) iff its Q > 0 there (and, for mS / mG, the
    sub-beam has melting; and, with per-gate weights, the weight is > 0).  Everything follows from the case's name;
  * presence(case, cols): that rule, from the columns alone;
  * accumulate(terms, present, weights): the operation by its definition, in NumPy;
  * CASES and the coverage they must have (coverage_failures).
tests/test_subsum_cpu.py pins accumulate to the oracle and asserts the coverage; tests/test_gpu_subsum.py pins the device."""
import functools
import zlib

import numpy as np

SPECIES = ('R', 'S', 'G', 'mS', 'mG', 'I')               # hydrometeor_list of the melting configuration, in its order
SPECIES_DRY = ('R', 'S', 'G')                            # ... without melting and ice crystals (Case.melt False)
Q_OF = {'R': 'QR_v', 'S': 'QS_v', 'G': 'QG_v', 'I': 'QI_v', 'mS': 'QmS_v', 'mG': 'QmG_v'}
VARS = ('U', 'V', 'W', 'QR_v', 'QS_v', 'QG_v', 'QI_v', 'RHO', 'T')

COUNTS = (2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 15, 16, 17, 25, 31, 32, 33, 49, 63, 64, 65, 81, 128, 129, 130)
SHAPES = ((1, 1), (1, 65), (2, 33), (3, 31), (5, 17), (8, 9), (15, 7), (16, 1), (16, 4), (17, 5), (33, 6))   # (rays, gates)
ALL_COUNT_SHAPES = ((17, 5), (3, 31))                    # every count runs at these
ALL_SHAPE_COUNTS = (4, 7, 49, 65, 130)                   # every shape runs at these

# presence families; 'chunks' (n_sub > 64 only) stands for two: absent tile-wide in all of chunk 0 in the first tile, and in
# all of chunk 1 in the last tile
FAMILIES = ('all', 'none', 'first', 'last', 'every2', 'every3', 'every5', 'rand50', 'rand05', 'one_lane', 'gap3_10', 'chunks')
TILE_GATES_LOG2 = 2                                      # CPOL_TILE_GATES_LOG2
WAVE = 64


def tile_shape(n_rays):
    """(rays, gates) of the tile a wavefront's lanes cover, as the host picks it: 16 x 4 from 16 rays on, else the gates
    doubled until the rays fit (8 x 8, 4 x 16, 2 x 32, 1 x 64)."""
    tl = TILE_GATES_LOG2
    while tl < 6 and (WAVE >> tl) > n_rays:
        tl += 1
    return WAVE >> tl, 1 << tl


class Case(object):
    """n_sub sub-beams of n_rays x n_gates; `rot` rotates the presence families over the species; `wgate`: per-gate weights
    with zeros (integration scheme 'ml'); `melt`: the melting configuration (False: R, S, G alone)."""

    def __init__(self, n_sub, n_rays, n_gates, rot, wgate=False, melt=True):
        self.n_sub, self.n_rays, self.n_gates, self.rot, self.wgate, self.melt = n_sub, n_rays, n_gates, rot, wgate, melt
        self.name = 's%d_r%d_g%d_p%d%s%s' % (n_sub, n_rays, n_gates, rot, '_wgate' if wgate else '', '' if melt else '_dry')
        self.species = SPECIES if melt else SPECIES_DRY

    def families(self):
        """{species: family}.  Six neighbouring families of the rotation; 'chunks' needs a second chunk and two tiles."""
        out = {}
        for j, h in enumerate(self.species):
            f = FAMILIES[(self.rot + j) % len(FAMILIES)]
            if (f == 'chunks' and (self.n_sub <= 64 or self.n_tiles() < 2)) or (f == 'gap3_10' and self.n_sub < 4):
                f = 'all'
            out[h] = f
        return out

    def n_tiles(self):
        tr, tg = tile_shape(self.n_rays)
        return -(-self.n_rays // tr) * -(-self.n_gates // tg)

    def tile_index(self):
        """[n_rays, n_gates] -> the tile (workgroup x index) of every gate, and its lane."""
        tr, tg = tile_shape(self.n_rays)
        gate_tiles = -(-self.n_gates // tg)
        r, g = np.meshgrid(np.arange(self.n_rays), np.arange(self.n_gates), indexing='ij')
        return (r // tr) * gate_tiles + g // tg, (r % tr) * tg + g % tg

    def drops_melting(self):
        return self.melt and self.rot % 3 == 0           # has_melting False on some sub-beams

    def __repr__(self):
        return self.name


def _case_list():
    cases, seen, rot = [], set(), 0

    def add(n_sub, shape, **kw):
        nonlocal rot
        key = (n_sub, shape, tuple(sorted(kw.items())))
        if key in seen:
            return
        seen.add(key)
        cases.append(Case(n_sub, shape[0], shape[1], rot, **kw))
        rot += 5                                         # (5 and 12 families are coprime: every rotation occurs)
    for shape in ALL_COUNT_SHAPES:
        for n in COUNTS:
            add(n, shape)
    for n in ALL_SHAPE_COUNTS:
        for shape in SHAPES:
            add(n, shape)
    # the remaining pairs that a pattern needs: a second chunk over many tiles of every shape with two tiles or more (the
    # 'chunks' family), and per-gate weights with zeros below, at and beyond one chunk and in the smallest tiles
    for n, shape in ((81, (33, 6)), (129, (8, 9)), (128, (15, 7)), (81, (2, 33))):
        add(n, shape)
    for n, shape in ((4, (5, 17)), (7, (17, 5)), (65, (17, 5)), (130, (3, 31)), (49, (33, 6)), (64, (1, 65))):
        add(n, shape, wgate=True)
    return cases


CASES = _case_list()
BY_NAME = {c.name: c for c in CASES}
# k_final evaluates 2 and 3 sub-beams in place only where that saves the k_psd_lookup launch: no melting species (2-D tables) and,
# with Doppler, no ice crystals (their table carries the Doppler sums)
DRY_CASES = [Case(n, r, g, rot, melt=False) for rot, (n, (r, g)) in
             enumerate([(n, sh) for n in (2, 3) for sh in ((17, 5), (3, 31), (1, 65))])]
# the Doppler sums of the sum kernels (Doppler scheme 2 with 1-moment ice)
DOPPLER_CASES = [Case(n, r, g, 4 + 5 * i) for i, (n, (r, g)) in
                 enumerate([(n, sh) for n in (4, 9, 65) for sh in ((17, 5), (1, 65))])]


def sub_weights(n_sub):
    """Distinct and of one magnitude (1 .. 1.4 over n_sub): any dropped, doubled or swapped sub-beam moves a sum of terms within
    a factor of 2 by more than 1 / (2 n_sub) of itself -- at least 3e-3 at 129 sub-beams, against bit equality (and 1e-5)."""
    s = np.arange(n_sub)
    w = (1.0 + 0.4 * ((7 * s) % 131) / 131.0) / n_sub
    assert len(np.unique(w)) == n_sub
    return w


def _pattern(case, family, rng):
    """bool [n_rays, n_sub, n_gates]"""
    nr, ns, ng = case.n_rays, case.n_sub, case.n_gates
    p = np.zeros((nr, ns, ng), dtype=bool)
    s = np.arange(ns)
    tile, _ = case.tile_index()
    if family == 'all':
        p[:] = True
    elif family == 'none':
        pass
    elif family == 'first':
        p[:, 0] = True
    elif family == 'last':
        p[:, ns - 1] = True
    elif family in ('every2', 'every3', 'every5'):
        p[:, s % int(family[5:]) == 1 % int(family[5:])] = True
    elif family == 'rand50':
        p[:] = rng.random(p.shape) < 0.5
    elif family == 'rand05':
        p[:] = rng.random(p.shape) < 0.05
        p[rng.integers(nr), rng.integers(ns), rng.integers(ng)] = True       # (never empty)
    elif family == 'one_lane':
        # one lane per tile, all of its sub-beams: the first gate of the tile in the order of (ray, gate), moved on by the tile
        for t in np.unique(tile):
            idx = np.argwhere(tile == t)
            r, g = idx[(3 * int(t) + 1) % len(idx)]
            p[r, :, g] = True
    elif family == 'gap3_10':
        p[:] = True
        first = tile == tile.min()
        p[:, 3:11][np.broadcast_to(first[:, None, :], p[:, 3:11].shape)] = False
    elif family == 'chunks':
        p[:] = True
        first, last = tile == tile.min(), tile == tile.max()
        p[:, :64][np.broadcast_to(first[:, None, :], p[:, :64].shape)] = False
        p[:, 64:][np.broadcast_to(last[:, None, :], p[:, 64:].shape)] = False
    else:
        raise ValueError(family)
    return p


@functools.lru_cache(maxsize=None)
def make_columns(case):
    """The columns of `case` (read-only arrays; computed once per case and shared)."""
    nr, ns, ng = case.n_rays, case.n_sub, case.n_gates
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    shape = (nr, ns, ng)
    s = np.arange(ns)
    sign = np.where(s % 2 == 0, 1.0, -1.0)[None, :, None]
    cols = {}
    # winds differing strongly between sub-beams: a sub-beam lost from RVEL's weighted mean moves it by metres per second
    cols['U'] = (20.0 * sign * (1.0 + 0.1 * rng.random(shape))).astype(np.float32)
    cols['V'] = (-15.0 * sign * (1.0 + 0.1 * rng.random(shape)) + 3.0).astype(np.float32)
    cols['W'] = (2.0 * sign * rng.random(shape)).astype(np.float32)
    cols['RHO'] = (0.6 + 0.6 * rng.random((nr, 1, ng)) + 0.01 * rng.random(shape)).astype(np.float32)
    # T and elevation vary across the tile: its lanes sit on many distinct (LUT slice, lambda panel) blocks
    cols['T'] = (205.0 + 75.0 * rng.random((nr, 1, ng)) + rng.uniform(-1.0, 1.0, shape)).astype(np.float32)
    el_ray = rng.uniform(0.3, 13.0, (nr, 1, 1))
    el_sub = rng.uniform(-0.7, 0.7, (1, ns, 1))
    elev = np.maximum(el_ray + el_sub + 0.02 * np.arange(ng)[None, None, :], 0.05)
    cols['elev'] = elev.astype(np.float32)
    cols['quad_pts'] = np.ascontiguousarray(np.stack(
        [np.broadcast_to(10.0 * np.arange(nr)[:, None] + rng.uniform(-0.7, 0.7, (1, ns)), (nr, ns)),
         np.broadcast_to((el_ray + el_sub)[:, :, 0], (nr, ns))], axis=-1))
    r, g = np.meshgrid(np.arange(nr), np.arange(ng), indexing='ij')
    code = np.zeros(shape, dtype=np.int8)
    code[(r[:, None, :] + 2 * s[None, :, None] + g[:, None, :]) % 5 == 0] = 1
    code[(r[:, None, :] + s[None, :, None] + 3 * g[:, None, :]) % 11 == 0] = -1
    cols['mask'] = code
    if case.wgate:
        w = sub_weights(ns)[None, :, None] * (1.0 + 0.2 * rng.random(shape))
        w[rng.random(shape) < 0.1] = 0.0
        w[:, 0][w.sum(axis=1) == 0] = 1.0 / ns                               # (every gate keeps a total > 0)
        cols['quad_weights'] = w
    else:
        cols['quad_weights'] = sub_weights(ns)
    fam = case.families()
    for h in case.species:
        # log-uniform over four decades across (ray, gate), within a factor of 2 across sub-beams
        q = 10.0 ** rng.uniform(-7.0, -3.0, (nr, 1, ng)) * rng.uniform(1.0, 2.0, shape)
        q = np.where(_pattern(case, fam[h], rng), q, 0.0)
        cols[Q_OF[h]] = q.astype(np.float32)
    for k in VARS:                                       # (the operator asks for every model variable of its list)
        cols.setdefault(k, np.zeros(shape, dtype=np.float32))
    # a few items beyond the integral tables (mass densities whose PSD slope leaves the tabulated range): rain and snow of two
    # gates, wherever they are present
    if nr * ng >= 20:
        for k, tiny in (('QR_v', 1e-16), ('QS_v', 3e-18)):
            for rr, gg in ((nr // 2, ng // 3), (nr - 1, ng - 1)):
                col = cols[k][rr, :, gg]
                cols[k][rr, :, gg] = np.where(col > 0, np.float32(tiny) * (1 + s % 5), 0).astype(np.float32)
    if case.melt:
        cols['fwet_mS'] = rng.uniform(0.02, 0.98, shape)
        cols['fwet_mG'] = rng.uniform(0.02, 0.98, shape)
        hm = np.ones((nr, ns), dtype=np.int8)
        if case.drops_melting():
            hm[(np.arange(nr)[:, None] + s[None, :]) % 4 == 1] = 0
        cols['has_melting'] = hm
    for a in cols.values():
        a.setflags(write=False)
    return cols


def presence(case, cols):
    """{species: bool [n_rays, n_sub, n_gates]} from the columns alone."""
    out = {}
    for h in case.species:
        p = cols[Q_OF[h]] > 0
        if h in ('mS', 'mG'):
            p = p & (cols['has_melting'][:, :, None] != 0)
        if np.ndim(cols['quad_weights']) == 3:
            p = p & (cols['quad_weights'] > 0)
        out[h] = p
    return out


def accumulate(terms, present, weights):
    """The sub-beam sum by its definition.  terms: float64 [n_sub, ..., n_columns]; present: bool [n_sub, ...]; weights:
    [n_sub], or per gate [n_sub, ...] over leading axes of `present` (then first divided by their sum over the sub-beams,
    added in the order of s).  Per entry the sum starts as NaN float32; for each sub-beam in order, where present:
    acc = float32(float64(0 if isnan(acc) else acc) + t) with t = terms * w in float64 and a NaN t counting as 0."""
    terms = np.asarray(terms, dtype=np.float64)
    present = np.asarray(present, dtype=bool)
    w = np.asarray(weights, dtype=np.float64)
    n_sub = terms.shape[0]
    assert present.shape == terms.shape[:-1] and w.shape[0] == n_sub and w.shape == present.shape[:w.ndim]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if w.ndim > 1:
            tot = np.zeros(w.shape[1:])
            for s in range(n_sub):
                tot = tot + w[s]
            w = w / tot
        w = w.reshape(w.shape + (1,) * (terms.ndim - w.ndim))
        acc = np.full(terms.shape[1:], np.nan, dtype=np.float32)
        for s in range(n_sub):
            t = terms[s] * w[s]
            t = np.where(np.isnan(t), 0.0, t)
            new = (np.where(np.isnan(acc), np.float32(0), acc).astype(np.float64) + t).astype(np.float32)
            acc = np.where(present[s][..., None], new, acc)
    return acc


def work_counts(case, pres):
    """{species: [n_tiles]} -- the number of sub-beams at which the species is present in at least one lane of the tile."""
    tile, _ = case.tile_index()
    out = {}
    for h, p in pres.items():
        ps = p.transpose(1, 0, 2)                        # [n_sub, n_rays, n_gates]
        out[h] = np.array([ps[:, tile == t].any(axis=1).sum() for t in np.unique(tile)])
    return out


def family_holds(case, family, p):
    """Whether the presence p [n_rays, n_sub, n_gates] of a species is of `family`, judged from p alone (with per-gate weights
    and dropped melting the families are thinned: those cases are judged on the species / sub-beams they leave alone)."""
    tile, _ = case.tile_index()
    ns = case.n_sub
    per_sub = p.any(axis=(0, 2))
    if family == 'all':
        return bool(p.all())
    if family == 'none':
        return not p.any()
    if family == 'first':
        return bool(p[:, 0].all()) and not p[:, 1:].any()
    if family == 'last':
        return bool(p[:, ns - 1].all()) and not p[:, :ns - 1].any()
    if family in ('every2', 'every3', 'every5'):
        k = int(family[5:])
        return bool(np.array_equal(per_sub, np.arange(ns) % k == 1 % k)) and bool(p[:, per_sub].all())
    if family in ('rand50', 'rand05'):
        d = p.mean()
        if p.size < 400:                                 # (too few entries to judge a density)
            return bool(p.any())
        return bool(0.35 < d < 0.65) if family == 'rand50' else bool(0 < d < 0.12)
    if family == 'one_lane':
        return all(p.any(axis=1)[tile == t].sum() == 1 and p.all(axis=1)[tile == t].sum() == 1 for t in np.unique(tile))
    first, last = tile == tile.min(), tile == tile.max()
    if family == 'gap3_10':
        gap = p[:, 3:11]
        return ns > 3 and not gap[np.broadcast_to(first[:, None, :], gap.shape)].any() and bool(p[:, :3].all()) and \
            bool(p[:, 11:].all()) and bool(gap[np.broadcast_to(~first[:, None, :], gap.shape)].all())
    if family == 'chunks':
        c0, c1 = p[:, :64], p[:, 64:]
        return ns > 64 and case.n_tiles() >= 2 and not c0[np.broadcast_to(first[:, None, :], c0.shape)].any() and \
            not c1[np.broadcast_to(last[:, None, :], c1.shape)].any() and \
            bool(c0[np.broadcast_to(~first[:, None, :], c0.shape)].all()) and \
            bool(c1[np.broadcast_to(~last[:, None, :], c1.shape)].all())
    raise ValueError(family)


def coverage_failures(cases=None):
    """What the case list must hold for the comparison on the device to mean something, from the columns alone."""
    cases = CASES if cases is None else cases
    bad = []
    fams, tiles, counts, shapes = set(), set(), set(), set()
    residues = {w: set() for w in range(2, 9)}
    dropped = wgate_zero = chunk0_skipped = chunk1_skipped = False
    for c in cases:
        cols = make_columns(c)
        pres = presence(c, cols)
        counts.add(c.n_sub)
        shapes.add((c.n_rays, c.n_gates))
        tiles.add(tile_shape(c.n_rays))
        clean = not c.wgate and not c.drops_melting()
        for h, f in c.families().items():
            if clean or (not c.wgate and h not in ('mS', 'mG')):
                if not family_holds(c, f, pres[h]):
                    bad.append('%s: %s is not of family %s' % (c.name, h, f))
                fams.add(f)
        for h, n in work_counts(c, pres).items():
            if c.n_sub >= 4:
                for w in residues:
                    residues[w] |= set((n % w).tolist())
        if c.drops_melting() and (cols['has_melting'] == 0).any():
            dropped = True
        if c.wgate and (cols['quad_weights'] == 0).any():
            wgate_zero = True
        if c.n_sub > 64:
            tile, _ = c.tile_index()
            for h, p in pres.items():
                ps = p.transpose(1, 0, 2)
                for t in np.unique(tile):
                    c0, c1 = ps[:64][:, tile == t].any(), ps[64:][:, tile == t].any()
                    chunk0_skipped |= bool(c1 and not c0)
                    chunk1_skipped |= bool(c0 and not c1)
    if fams != set(FAMILIES):
        bad.append('families never staged: %s' % sorted(set(FAMILIES) - fams))
    if tiles != {(16, 4), (8, 8), (4, 16), (2, 32), (1, 64)}:
        bad.append('tile shapes %s' % sorted(tiles))
    if counts != set(COUNTS) or shapes != set(SHAPES):
        bad.append('counts or shapes missing')
    for w, r in residues.items():
        if r != set(range(w)):
            bad.append('the sub-beams with work in a tile never number %s mod %d' % (sorted(set(range(w)) - r), w))
    if set(n % 7 for n in counts) != set(range(7)):
        bad.append('the counts miss a residue mod 7')
    for ok, what in ((dropped, 'has_melting False'), (wgate_zero, 'a per-gate weight of 0'),
                     (chunk0_skipped, 'a tile whose species is absent in all of chunk 0 and present in chunk 1'),
                     (chunk1_skipped, 'a tile whose species is present in chunk 0 and absent in all of chunk 1')):
        if not ok:
            bad.append('never staged: ' + what)
    for c in cases:
        if c.n_rays * c.n_sub * c.n_gates > 33 * 130 * 6:
            bad.append('%s is larger than 33 x 130 x 6 sub-beam gates' % c.name)
    return bad


def oracle_subbeams(case, cols, ray, radial_res=600.0):
    """The oracle's sub-radials of one ray of the columns (fresh arrays: the oracle folds elevations in place)."""
    from cosmo_pol_oracle.beam import SubBeam
    ng = case.n_gates
    w = cols['quad_weights']
    subs = []
    for s in range(case.n_sub):
        values = {k: np.array(cols[k][ray, s], dtype=np.float32) for k in VARS if k in cols}
        if case.melt:
            for k in ('QmS_v', 'QmG_v'):
                values[k] = np.array(cols[k][ray, s], dtype=np.float64)
            for k in ('fwet_mS', 'fwet_mG'):
                values[k] = np.array(cols[k][ray, s], dtype=np.float64)
        sb = SubBeam(values, cols['mask'][ray, s].astype(np.float64), np.zeros(ng), np.zeros(ng),
                     radial_res * (0.5 + np.arange(ng)), np.zeros(ng), elev=np.array(cols['elev'][ray, s], dtype=np.float32),
                     quad_pt=[float(x) for x in cols['quad_pts'][ray, s]],
                     quad_weight=(np.array(w[ray, s]) if np.ndim(w) == 3 else np.float64(w[s])))
        if case.melt:
            sb.has_melting = bool(cols['has_melting'][ray, s])
        subs.append(sb)
    return subs
