"""Inputs and a plain reference for the level search of the gate kernel (gate_geometry, cosmo_pol_amd/csrc/cpol_interp.inl).

The device finds the level index of a gate in one of three ways, chosen by the number of model levels nz: a bisection
(nz = 3 or nz > 144), a "wide" count over every 16th level and four 4-float windows (nz = 4 .. 81), and the same with a
second group of sixteenths (nz = 82 .. 144).  Here are
  * rough_cube: a small cube whose neighbour columns lie many levels apart (a 2500 m checkerboard under three different
    model tops), so that the walk from column 0's answer to the other three columns takes many steps;
  * points: positions and heights on every comparison that decides index, -9999 and NaN -- every level height of the four
    neighbour columns and its float32 neighbours, the column tops, the blended topography, grid nodes, the domain edges;
  * reference_points: the gate kernel restated in NumPy float32, statement by statement as oracle/interp_twin.c has it,
    with the level index by its DEFINITION (a count over the column) instead of any search.
tests/test_levels_cpu.py pins the restatement to the C twin; tests/test_gpu_levels.py pins the device to both."""
import functools

import numpy as np

from cosmo_pol_amd import synthetic

# both sides of every threshold of the search (the count of sixteenths flips at nz = 18, 34, 50, 66, 82, 98, 114, 130), the
# boundaries of its three forms (3 | 4, 81 | 82, 144 | 145), the clamped windows (nz = 4 .. 7) and one size far beyond them
NZ_POINTS = [3, 4, 5, 6, 7, 8, 17, 18, 19, 20, 33, 34, 65, 66, 80, 81, 82, 83,
             97, 98, 113, 114, 129, 130, 143, 144, 145, 146, 160, 257]
NY, NX = 10, 11
RES = 0.02
LLC = (-1.0, -0.5)                       # (lon, lat) of the lower left corner
SOUTH_POLE = [-43.0, 10.0]
TOPS = np.array([21000.0, 22500.0, 24000.0], dtype=np.float32)
CHECKER = np.float32(2500.0)

F32 = np.float32
_UP, _DOWN = F32(np.inf), F32(-np.inf)


def roughen(zlevels):
    """z-levels [nz, ny, nx] rebuilt as topo2 + (top - topo2) * eta: eta is synthetic.make_cube's own formula, topo2 the
    cube's lowest level plus a 2500 m checkerboard over (i + j) % 2, top a model top of 21 000, 22 500 or 24 000 m per
    column, chosen by (i + 2 j) % 3 (every 2 x 2 neighbourhood has all three).  Columns descend strictly."""
    nz, ny, nx = zlevels.shape
    ii, jj = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    topo2 = (zlevels[-1] + CHECKER * ((ii + jj) % 2).astype(np.float32)).astype(np.float32)
    top = TOPS[(ii + 2 * jj) % 3]
    eta = ((nz - np.arange(nz) - 0.5) / nz).astype(np.float64) ** 1.5
    z = (topo2[None] + (top - topo2)[None] * eta.astype(np.float32)[:, None, None]).astype(np.float32)
    assert np.all(z[:-1] > z[1:]), 'columns must descend strictly'
    return z


def rough_cube(nz, ny=NY, nx=NX, seed=0):
    cube = synthetic.make_cube(nz=nz, ny=ny, nx=nx, res=RES, llc=LLC, seed=seed)
    cube['zlevels'] = roughen(cube['zlevels'])
    return cube


def grid_of(cube):
    """(llc, urc, res) as float32 pairs (lon, lat), formed as RadarOperator._stage_model forms them."""
    p = cube['proj_info']
    llc = np.asarray((float(p['Lo1']), float(p['La1']))).astype(np.float32)
    urc = np.asarray((float(p['Lo2']), float(p['La2']))).astype(np.float32)
    return llc, urc, np.asarray(cube['resolution'], dtype=np.float32)


def _position(coords, llc, res):
    """interp_twin.c:55-62 for coords [n, 2] (lat, lon): the cell (i0, i1) and the weights x, y, dx, dy."""
    coords = np.asarray(coords, dtype=np.float32)
    p0 = (coords[:, 0] - llc[1]) / res[1]                       # float32 quotients
    p1 = (coords[:, 1] - llc[0]) / res[0]
    assert p0.dtype == np.float32 and p1.dtype == np.float32
    i0 = np.floor(p0.astype(np.float64)).astype(np.int64)
    i1 = np.floor(p1.astype(np.float64)).astype(np.int64)
    x = np.fmod(p0.astype(np.float64), 1.0).astype(np.float32)
    y = np.fmod(p1.astype(np.float64), 1.0).astype(np.float32)
    dx = (1.0 - x.astype(np.float64)).astype(np.float32)
    dy = (1.0 - y.astype(np.float64)).astype(np.float32)
    return i0, i1, x, y, dx, dy


def _neighbours(i0, i1, ny, nx):
    """The four neighbour columns (i0, i1) (i0, i1 + 1) (i0 + 1, i1) (i0 + 1, i1 + 1), clamped to the grid as the device clamps
    them, and whether the unclamped indices lie inside it (where they do not, the C twin reads past its arrays)."""
    ni = np.stack([i0, i0, i0 + 1, i0 + 1], axis=1)
    nj = np.stack([i1, i1 + 1, i1, i1 + 1], axis=1)
    interior = np.all((ni >= 0) & (ni <= ny - 1) & (nj >= 0) & (nj <= nx - 1), axis=1)
    return np.clip(ni, 0, ny - 1), np.clip(nj, 0, nx - 1), interior


def _blend(x, y, dx, dy, t):
    """interp_twin.c:70 / :86: dx dy t0 + x t2 dy + dx t1 y + x y t3, float32, in this order."""
    return dx * dy * t[..., 0] + x * t[..., 2] * dy + dx * t[..., 1] * y + x * y * t[..., 3]


def reference_points(data, zlevels, llc, res, coords, heights, chunk=16384):
    """get_all_radar_pts in NumPy float32 (`data` [nz, ny, nx], or several variables at once [n_vars, nz, ny, nx]: then
    'values' is [n_vars, n]).  Returns a dict: 'values' [n] (NaN below the blended topography, -9999 above a
    column top), 'status' [n] (0 a value, +1 above, -1 below), 'index' [n, 4] (per neighbour column the largest i in
    [0, nz - 2] with col[i] >= h, 0 if none: a count, defined for every point), 'above' / 'below' [n, 4] (h over the column's
    top / under its lowest level: the twin's -1 / -2), 'c1' [n, 4], 'topo' [n], 'x', 'y' [n] and 'interior' [n]."""
    data = np.asarray(data, dtype=np.float32)
    zl = np.asarray(zlevels, dtype=np.float32)
    llc = np.asarray(llc, dtype=np.float32)
    res = np.asarray(res, dtype=np.float32)
    coords = np.asarray(coords, dtype=np.float32)
    heights = np.asarray(heights, dtype=np.float32)
    nz, ny, nx = zl.shape
    n = heights.shape[0]
    assert data.shape[-3:] == zl.shape
    out = {'values': np.empty(data.shape[:-3] + (n,), np.float32), 'status': np.empty(n, np.int8), 'index': np.empty((n, 4), np.int32),
           'above': np.empty((n, 4), bool), 'below': np.empty((n, 4), bool), 'c1': np.empty((n, 4), np.int32),
           'topo': np.empty(n, np.float32), 'x': np.empty(n, np.float32), 'y': np.empty(n, np.float32),
           'interior': np.empty(n, bool)}
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, n, chunk):
            sl = slice(a, min(a + chunk, n))
            h = heights[sl]
            i0, i1, x, y, dx, dy = _position(coords[sl], llc, res)
            ni, nj, interior = _neighbours(i0, i1, ny, nx)
            topo = _blend(x, y, dx, dy, zl[nz - 1, ni, nj])
            ground = ~(topo < h)                                          # (NaN heights: below)
            col = zl[:, ni, nj]                                           # [nz, m, 4]
            above = h[:, None] > col[0]
            below = h[:, None] < col[nz - 1]
            # the index by its definition: levels 1 .. nz - 2 at or above the gate (columns descend strictly)
            index = np.sum(col[1:nz - 1] >= h[None, :, None], axis=0).astype(np.int32)
            c1 = np.where(below, nz - 3, np.minimum(index, nz - 3)).astype(np.int32)
            z1, z2 = zl[c1, ni, nj], zl[c1 + 1, ni, nj]
            v1, v2 = data[..., c1, ni, nj], data[..., c1 + 1, ni, nj]
            v = v2 - (v2 - v1) / (z1 - z2) * (h[:, None] - z2)            # interp_twin.c:84, float32
            assert v.dtype == np.float32
            val = _blend(x, y, dx, dy, v)
            high = above.any(axis=1)
            val = np.where(high, np.float32(-9999.0), val)
            val = np.where(ground, np.float32(np.nan), val).astype(np.float32)
            out['values'][..., sl] = val
            out['status'][sl] = np.where(ground, -1, np.where(high, 1, 0))
            out['index'][sl], out['above'][sl], out['below'][sl], out['c1'][sl] = index, above, below, c1
            out['topo'][sl], out['x'][sl], out['y'][sl], out['interior'][sl] = topo, x, y, interior
    return out


def _cell_edges(lo, r, n):
    """For i = 1 .. n - 1 the smallest float32 coordinate c with floor((c - lo) / r) >= i (the float32 quotient the kernel
    forms): the lower edge of cell i as the kernel sees it.  -> {i: c}"""
    out = {}
    for i in range(1, n):
        c = F32(np.float64(lo) + np.float64(r) * i)
        q = lambda v: np.floor(np.float64((F32(v) - lo) / r))
        while q(c) >= i:
            c = np.nextafter(c, _DOWN)
        while q(c) < i:
            c = np.nextafter(c, _UP)
        out[i] = F32(c)
    return out


def positions(cube, seed):
    """Horizontal positions [m, 2] (lat, lon) float32: 64 uniform inside the grid; grid nodes (the lower edges of cells, with
    both fractions exactly 0 where the float32 quotient allows it -- always at node (0, 0)); one float32 below such edges;
    row 0 and column 0; the upper edge urc and one float32 below it."""
    llc, urc, res = grid_of(cube)
    nz, ny, nx = cube['zlevels'].shape
    rng = np.random.default_rng(seed)
    lat_e, lon_e = _cell_edges(llc[1], res[1], ny), _cell_edges(llc[0], res[0], nx)
    lat_u = lambda k: rng.uniform(llc[1], lat_e[ny - 1], k).astype(np.float32)
    lon_u = lambda k: rng.uniform(llc[0], lon_e[nx - 1], k).astype(np.float32)
    pos = [np.stack([lat_u(64), lon_u(64)], axis=1)]
    # nodes: first those where the quotient is an integer, then others, 3 per axis
    frac0 = lambda c, lo, r: np.fmod(np.float64((F32(c) - lo) / r), 1.0) == 0.0
    def pick(edges, lo, r, n):
        exact = [i for i in range(1, n - 1) if frac0(edges[i], lo, r)]
        rest = [i for i in range(1, n - 1) if i not in exact]
        rng.shuffle(rest)
        return (exact + rest)[:3]
    ii, jj = pick(lat_e, llc[1], res[1], ny), pick(lon_e, llc[0], res[0], nx)
    nodes = [(llc[1], llc[0])] + [(lat_e[i], lon_e[j]) for i, j in zip(ii, jj)]
    pos.append(np.array(nodes, dtype=np.float32))
    below = [(np.nextafter(lat_e[i], _DOWN), np.nextafter(lon_e[j], _DOWN)) for i, j in zip(ii, jj)]
    below += [(np.nextafter(lat_e[ii[0]], _DOWN), lon_u(1)[0]), (lat_u(1)[0], np.nextafter(lon_e[jj[0]], _DOWN))]
    pos.append(np.array(below, dtype=np.float32))
    pos.append(np.stack([np.full(2, llc[1], np.float32), lon_u(2)], axis=1))              # row 0
    pos.append(np.stack([lat_u(2), np.full(2, llc[0], np.float32)], axis=1))              # column 0
    lat_b, lon_b = np.nextafter(urc[1], _DOWN), np.nextafter(urc[0], _DOWN)
    edge = [(urc[1], lon_u(1)[0]), (lat_u(1)[0], urc[0]), (urc[1], urc[0]),
            (lat_b, lon_u(1)[0]), (lat_u(1)[0], lon_b), (lat_b, lon_b)]
    pos.append(np.array(edge, dtype=np.float32))
    return np.concatenate(pos).astype(np.float32)


def points(cube, seed):
    """-> (coords [n, 2] float32, heights [n] float32, interior [n] bool).  At every position of positions(): every level
    height of the four neighbour columns and its float32 neighbours above and below (the column tops with them), the
    blended topography +- 1 ulp, three heights between the blend and the lowest level of the highest neighbour column, 32
    heights uniform in [-500 m, top + 500 m], NaN, +inf and -inf."""
    llc, urc, res = grid_of(cube)
    zl = cube['zlevels']
    nz, ny, nx = zl.shape
    rng = np.random.default_rng(seed + 1)
    pos = positions(cube, seed)
    i0, i1, x, y, dx, dy = _position(pos, llc, res)
    ni, nj, interior = _neighbours(i0, i1, ny, nx)
    topo = _blend(x, y, dx, dy, zl[nz - 1, ni, nj])
    coords, heights, inside = [], [], []
    for p in range(pos.shape[0]):
        lev = zl[:, ni[p], nj[p]].ravel()
        low = zl[nz - 1, ni[p], nj[p]].max()
        top = zl[0, ni[p], nj[p]].max()
        h = [lev, np.nextafter(lev, _UP), np.nextafter(lev, _DOWN),
             np.array([topo[p], np.nextafter(topo[p], _UP), np.nextafter(topo[p], _DOWN)], dtype=np.float32),
             (topo[p] + (low - topo[p]) * np.array([0.25, 0.5, 0.75], dtype=np.float32)).astype(np.float32),
             rng.uniform(-500.0, float(top) + 500.0, 32).astype(np.float32),
             np.array([np.nan, np.inf, -np.inf], dtype=np.float32)]
        h = np.concatenate(h).astype(np.float32)
        heights.append(h)
        coords.append(np.broadcast_to(pos[p], (h.shape[0], 2)))
        inside.append(np.full(h.shape[0], interior[p]))
    return (np.ascontiguousarray(np.concatenate(coords), dtype=np.float32), np.concatenate(heights),
            np.concatenate(inside))


@functools.lru_cache(maxsize=3)
def case(nz):
    """The cube, points and restatement of one level count, shared by the tests of that level count and never edited (the
    arrays are read-only; the largest case holds ~40 MB, so only the last few are kept):
    -> dict(cube, llc, urc, res, second, coords, heights, interior, ref (of T), ref2 (of `second`))."""
    cube = rough_cube(nz, seed=1000 + nz)
    llc, urc, res = grid_of(cube)
    coords, heights, interior = points(cube, seed=nz)
    second = np.random.default_rng(nz).normal(size=cube['zlevels'].shape).astype(np.float32)
    ref = reference_points(cube['data']['T'], cube['zlevels'], llc, res, coords, heights)
    ref2 = reference_points(second, cube['zlevels'], llc, res, coords, heights)
    assert np.array_equal(ref['interior'], interior)
    for a in (coords, heights, interior, second, cube['zlevels'], cube['data']['T'], ref['values'], ref2['values']):
        a.setflags(write=False)
    return dict(cube=cube, llc=llc, urc=urc, res=res, second=second, coords=coords, heights=heights, interior=interior,
                ref=ref, ref2=ref2)


def coverage_failures(nz, ref):
    """The conditions a cube's points must meet for the comparison to mean something, from the restatement alone."""
    st, idx = ref['status'], ref['index']
    ok = st == 0
    bad = []
    missing = sorted(set(range(nz - 1)) - set(np.unique(idx[ok, 0]).tolist()))
    if missing:
        bad.append("column 0's index never takes %s" % missing[:8])
    for s, name in ((0, 'a value'), (-1, 'NaN'), (1, '-9999')):
        if not (st == s).any():
            bad.append('no point with ' + name)
    n_above = ref['above'].sum(axis=1)
    if not ((n_above > 0) & (n_above < 4) & (st == 1)).any():
        bad.append('no point above the top of some but not all of its columns')
    if not (ok & ref['below'].any(axis=1)).any():
        bad.append('no point below a lowest level yet above the blended topography (c1 = nz - 3 extrapolation)')
    if not (ok & (ref['x'] == 0) & (ref['y'] == 0)).any():
        bad.append('no valued point on a grid node (both fractions 0)')
    if not (ok & ~ref['interior']).any():
        bad.append('no valued point on the upper domain edge')
    if nz >= 65:
        d = idx[ok, 1:] - idx[ok, :1]
        if not (d >= 8).any():
            bad.append('no neighbour column >= 8 levels above column 0 (largest %d)' % d.max())
        if not (d <= -8).any():
            bad.append('no neighbour column >= 8 levels below column 0 (smallest %d)' % d.min())
    if 3 * ok.sum() < st.size:
        bad.append('only %d of %d points carry a value' % (ok.sum(), st.size))
    return bad


def same_bits(a, b):
    """float32 arrays equal as uint32 words where neither is NaN, and NaN at the same places."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def first_differences(got, ref, heights, coords, k=5):
    """A short report of where two float32 result arrays differ (for assertion messages)."""
    got, want = np.asarray(got), np.asarray(ref['values'])
    diff = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    w = np.where(diff)[0]
    return '%d of %d points differ; first: %s' % (w.size, got.size, [
        dict(i=int(i), got=float(got[i]), want=float(want[i]), h=float(heights[i]), lat=float(coords[i, 0]),
             lon=float(coords[i, 1]), index=ref['index'][i].tolist(), status=int(ref['status'][i])) for i in w[:k]])


# ---------------------------------------------------------------- sweeps over rough cubes
NZ_SWEEP = [3, 4, 19, 82, 98, 144, 145]
SWEEP_CASES = ('c3_melt_ice', 'c4_7x7')           # one beam / 7 x 7 sub-beams
SWEEP_ELEVATIONS = (30.0, 75.0)                   # besides the case's own: gates cross every level and leave the model top


@functools.lru_cache(maxsize=4)
def sweep_case(name, nz):
    """An end-to-end radial case (tests/_cases.py) on its own cube at `nz` levels with roughened z-levels: -> dict(over, conf, luts,
    cube, ocube, rays [(az, el)], subs [per ray the oracle's sub-radials], blocks (the 16-level blocks column 0's index falls
    into under the gates), masks (the mask codes that occur)).  Computed once; the sub-radials are never edited."""
    import _cases
    import gen_golden
    from cosmo_pol_oracle import beam
    hyds, two = gen_golden.RADIAL_CASES[name][3:]
    conf, az, el, _, luts, _ = _cases.radial_case(name)
    over = gen_golden.radial_case_inputs(name)[0]
    cube = synthetic.small_test_cube(hydrometeors=hyds, two_moment=two, **dict(gen_golden.CUBE_KW, nz=nz))
    cube['zlevels'] = roughen(cube['zlevels'])
    order = _cases.ORDER_2MOM if two else _cases.ORDER
    ocube = beam.ModelCube({n: cube['data'][n].copy() for n in order}, cube['zlevels'], cube['proj_info'], cube['resolution'],
                           order)
    rays = [(az, el)] + [(az, e) for e in SWEEP_ELEVATIONS]
    subs = [beam.interpolate_radial(ocube, conf, a, e) for a, e in rays]
    blocks, masks = set(), set()
    for per_ray in subs:
        for sb in per_ray:
            rc = beam.gate_coordinates(ocube, conf['radar']['coords'], sb.quad_pt[0], sb.dist_profile)[2]
            ref = reference_points(cube['data'][order[0]], cube['zlevels'], ocube.llc, ocube.resolution, rc, sb.heights_profile)
            assert np.array_equal(ref['status'], sb.mask)
            blocks |= set((ref['index'][ref['status'] == 0, 0] // 16).tolist())
            masks |= set(int(m) for m in np.unique(sb.mask))
    return dict(over=over, conf=conf, luts=luts, cube=cube, ocube=ocube, rays=rays, subs=subs, blocks=blocks, masks=masks)


def sweep_coverage_failures(nz, case):
    bad = []
    missing = sorted(set(range((nz - 2) // 16 + 1)) - case['blocks'])
    if missing:
        bad.append("column 0's index under the gates never falls into the 16-level blocks %s" % missing)
    if case['masks'] != {-1, 0, 1}:
        bad.append('mask codes %s' % sorted(case['masks']))
    return bad
