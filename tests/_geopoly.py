"""Host model and scenarios of the COORDINATE POLYNOMIALS (cpol_interp.inl: k_trajectory's fit, interp_gate's Horner chains and
guard).  NumPy float64 only, no GPU: tests/test_geo_poly_cpu.py checks the model and the scenarios on their own, and
tests/test_gpu_geo_poly.py holds the device against them.

  host_fit      per (ray, horizontal node): the 9 Chebyshev-node values of the rotated latitude / longitude (Vincenty's direct
                formula of cosmo_pol_oracle.geodesy, the rotation in float64), the monomial coefficients the device forms
                from them, and the verdicts of the two sanity rules -- `sane_nodes` (node values finite, neighbours at most a
                degree apart: the only rule before this module existed) and `sane` (that, and the fit's two highest Chebyshev
                coefficients at most 2^-26 of the smallest node value: the rule of k_trajectory now)
  exact_coords  float64 rotated coordinates of every sub-beam gate from the float32 arc distances of the debug read `traj`
  scenario      a configuration, a cube and the rays (one hydrometeor, at most 48 rays x 100 gates, 12 levels)
"""
import copy

import numpy as np

from cosmo_pol_amd import geometry, quadrature, synthetic
from cosmo_pol_oracle import geodesy

NP = 9
DEG = np.pi / 180.0
NODES = np.cos(np.pi * (np.arange(NP) + 0.5) / NP)              # x_q, descending: x_0 = cos(pi / 18)
RULE_NODE_STEP = 1.0                                            # degrees between neighbouring nodes
RULE_TAIL = 2.0 ** -26                                          # (|c7| + |c8|) / min |node value|: less than 1 / 4 of that value's float32 ulp
SITE = (46.5, 7.5, 1000.0)                                      # (bench.bench_config)
POLE = (-43.0, 10.0)
HYDS = ('R',)                                                   # in the cubes
TABLES = ('R', 'S', 'G')                                        # what a 1-moment configuration asks tables for
SHAPES = [(3, 3, 9), (3, 3, 19), (7, 7, 4), (7, 7, 8), (5, 1, 1), (5, 1, 6), (29, 1, 1), (29, 1, 3), (3, 3, 1)]
# n_rays * n_h = 27, 57 | 28, 56 | 5, 30 | 29, 87 | 3: one below, at and one above the 28 fits of a workgroup and of two; (29, 1) is the only
# shape whose grid (n_rays * n_v workgroups of 28 fits) is smaller than its fits, i.e. where the fit's stride loop runs twice


def _fit_matrix():
    """Node values -> monomial coefficients, as cpol_run_sweep builds it (long double, rounded to float64): M[power, node]."""
    T = np.zeros((NP, NP), dtype=np.longdouble)
    T[0, 0] = 1
    T[1, 1] = 1
    for k in range(2, NP):
        T[k, 1:] = 2 * T[k - 1, :-1]
        T[k] -= T[k - 2]
    pi = np.longdouble('3.141592653589793238462643383279502884')
    q = np.arange(NP, dtype=np.longdouble)
    M = np.zeros((NP, NP), dtype=np.longdouble)
    for pw in range(NP):
        for k in range(NP):
            M[pw] += T[k, pw] * (1 if k == 0 else 2) / np.longdouble(NP) * np.cos(pi * k * (q + np.longdouble(0.5)) / NP)
    return M.astype(np.float64)


FIT_M = _fit_matrix()


def rotate64(lat_deg, lon_deg, south_pole):
    """geodesy.wgs_to_rotated without its float32 cast: (rotated latitude, rotated longitude) in float64 degrees."""
    r = geodesy.rotation_constants(south_pole[0], south_pole[1])
    lat = np.asarray(lat_deg, dtype=np.float64) * DEG
    lon = np.asarray(lon_deg, dtype=np.float64) * DEG
    cl = np.cos(lat)
    x, y, z = np.cos(lon) * cl, np.sin(lon) * cl, np.sin(lat)
    x_new = r['ct'] * r['cp'] * x + r['ct'] * r['sp'] * y + r['st'] * z
    y_new = -r['sp'] * x + r['cp'] * y
    z_new = -r['st'] * r['cp'] * x - r['st'] * r['sp'] * y + r['ct'] * z
    return np.arcsin(np.clip(z_new, -1.0, 1.0)) / DEG, np.arctan2(y_new, x_new) / DEG


def exact_at(site, south_pole, az_deg, s):
    """Rotated coordinates [..., 2] = (rlat, rlon), float64, at arc distances s [m] along the geodesics that leave the site
    under az_deg (broadcast against s)."""
    az_deg, s = np.broadcast_arrays(np.asarray(az_deg, np.float64), np.asarray(s, np.float64))
    lat, lon = geodesy.wgs84_direct(site[0], site[1], az_deg, s)
    return np.stack(rotate64(lat, lon, south_pole), axis=-1)


def s_max_of(conf):
    """1.001 x the slant range of the last gate: 2 / poly_scale of cpol_run_sweep."""
    r = conf['radar']
    n_gates = len(np.arange(r['radial_resolution'] / 2., r['range'], r['radial_resolution']))
    return 1.001 * (r['radial_resolution'] / 2. + (n_gates - 1) * r['radial_resolution'])


def node_azimuths(conf, az):
    """[n_rays, n_h] azimuths (degrees) of the horizontal quadrature nodes: the operator's own quadrature and the expression of
    geometry.ray_tables."""
    sub = quadrature.subbeams(conf)
    return sub.pts_hor[None, :] + np.asarray(az, np.float64).reshape(-1)[:, None]


def host_fit(site, south_pole, azimuths_of_the_horizontal_nodes, s_max):
    """dict of: `nodes` [n_rays, n_h, 2, 9] float64 (rlat, rlon at the Chebyshev nodes, s = (x_q + 1) s_max / 2), `coef`
    [n_rays, n_h, 2, 9] monomial coefficients in x, `cheb_tail` [n_rays, n_h, 2] = |c7| + |c8|, `node_step` [n_rays, n_h] the
    largest difference of neighbouring node values, `sane_nodes` and `sane` [n_rays, n_h] bool."""
    az = np.asarray(azimuths_of_the_horizontal_nodes, np.float64)
    s = (NODES + 1.0) * (s_max / 2.0)
    v = exact_at(site, south_pole, az[..., None], s)                       # [n_rays, n_h, 9, 2]
    nodes = np.ascontiguousarray(np.moveaxis(v, -1, -2))                    # [n_rays, n_h, 2, 9]
    coef = np.einsum('pq,...q->...p', FIT_M, nodes)
    step = np.abs(np.diff(nodes, axis=-1)).max(axis=(-1, -2))
    finite = np.isfinite(nodes).all(axis=(-1, -2))
    sane_nodes = finite & (step <= RULE_NODE_STEP)
    # the Chebyshev coefficients c7, c8 from the monomial ones: T8 = 128 x^8 - ..., T7 = 64 x^7 - ..., T8 has no x^7
    tail = np.abs(coef[..., 7]) / 64.0 + np.abs(coef[..., 8]) / 128.0       # [n_rays, n_h, 2]
    smallest = np.abs(nodes).min(axis=-1)
    sane = sane_nodes & (tail <= RULE_TAIL * smallest).all(axis=-1)
    return dict(nodes=nodes, coef=coef, cheb_tail=tail, node_step=step, sane_nodes=sane_nodes, sane=sane)


def tail_ratio(fit):
    """[n_rays, n_h]: the larger of (|c7| + |c8|) / (2^-26 min |node value|) over the two coordinates; the tail rule accepts <= 1."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return (fit['cheb_tail'] / (RULE_TAIL * np.abs(fit['nodes']).min(axis=-1))).max(axis=-1)


def poly_at(coef, s, s_max):
    """The fits' values at arc distances s [n_rays, n_gates] (float64 Horner in x = 2 s / s_max - 1) -> [n_rays, n_h, n_gates, 2]."""
    x = 2.0 * np.asarray(s, np.float64) / s_max - 1.0
    x = x[:, None, None, :]
    acc = np.zeros(coef.shape[:3] + (x.shape[-1],))
    for q in range(NP - 1, -1, -1):
        acc = acc * x + coef[..., q][..., None]
    return np.moveaxis(acc, 2, -1)


def exact_coords(site, south_pole, azimuths_of_the_horizontal_nodes, s32, sub_h, sub_v):
    """float64 (rlat, rlon) [n_rays, n_sub, n_gates, 2] of every sub-beam gate: s32 [n_rays, n_v, n_gates] are the float32 arc
    distances of the debug read `traj`, sub-beam k sits on horizontal node sub_h[k] and vertical node sub_v[k]."""
    az = np.asarray(azimuths_of_the_horizontal_nodes, np.float64)
    s = np.asarray(s32).astype(np.float64)[:, np.asarray(sub_v)]            # [n_rays, n_sub, n_gates]
    return exact_at(site, south_pole, az[:, np.asarray(sub_h)][..., None], s)


def ulp32(v):
    """Spacing of float32 at |v| (v float64 or float32)."""
    return np.spacing(np.abs(np.asarray(v)).astype(np.float32)).astype(np.float64)


def ulp_distance(a, b):
    """Float32 values apart in units in the last place (0 = same bits or +-0); NaN where either is NaN -> a huge number."""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def cell_index(coords, proj, res):
    """(i0, i1) as gate_geometry computes them (tools/fast_sub_check.py::cell_index): float32 quotient, floor.  coords [..., 2]."""
    c = np.asarray(coords, np.float32)
    p0 = (c[..., 0] - np.float32(proj['La1'])) / np.float32(res[1])
    p1 = (c[..., 1] - np.float32(proj['Lo1'])) / np.float32(res[0])
    with np.errstate(invalid='ignore'):
        return np.floor(p0.astype(np.float64)), np.floor(p1.astype(np.float64))


def border_gates(exact, proj, res):
    """bool [...]: gates whose exact coordinate lies within 2 float32 ulp of a cell border or of the domain border, in either
    direction (the coordinates at which two correct float32 roundings may sit in different cells)."""
    out = np.zeros(exact.shape[:-1], bool)
    for j, (lo, hi, r) in enumerate(((proj['La1'], proj['La2'], res[1]), (proj['Lo1'], proj['Lo2'], res[0]))):
        c = exact[..., j]
        lo32, hi32, r32 = float(np.float32(lo)), float(np.float32(hi)), float(np.float32(r))
        d = 2.0 * ulp32(np.maximum(np.abs(c), abs(lo32)))
        t = (c - lo32) / r32
        near_cell = np.abs(t - np.round(t)) * r32 <= d
        out |= near_cell | (np.abs(c - lo32) <= d) | (np.abs(c - hi32) <= d)
    return out


def in_domain(exact, proj):
    return ((exact[..., 0] >= float(np.float32(proj['La1']))) & (exact[..., 0] <= float(np.float32(proj['La2'])))
            & (exact[..., 1] >= float(np.float32(proj['Lo1']))) & (exact[..., 1] <= float(np.float32(proj['Lo2']))))


# ------------------------------------------------------------------------------------------------------------------ scenarios
def _conf(site, rng, step, nh=3, nv=3):
    return {'radar': {'coords': [float(site[0]), float(site[1]), float(site[2])], 'frequency': 5.6, 'range': rng,
                      'radial_resolution': step, '3dB_beamwidth': 1., 'K_squared': 0.93, 'type': 'ground',
                      'sensitivity': [-5, 10000]},
            'refraction': {'scheme': 1},
            'integration': {'scheme': 1, 'nh_GH': nh, 'nv_GH': nv, 'weight_threshold': 1.},
            'doppler': {'scheme': 1},
            'microphysics': {'scheme': '1mom', 'with_melting': 0, 'with_ice_crystals': 0, 'with_attenuation': 1}}


def _cube(lat_lo, lat_hi, lon_lo, lon_hi, dlat, dlon, pole, nz=8):
    """synthetic.make_cube's dictionary on a grid whose two resolutions may differ (rain and the wind: smooth functions of the
    cell indices, so that a gate read from a neighbouring cell differs)."""
    ny = int(round((lat_hi - lat_lo) / dlat)) + 1
    nx = int(round((lon_hi - lon_lo) / dlon)) + 1
    if dlat == dlon:
        return synthetic.make_cube(nz=nz, ny=ny, nx=nx, res=dlat, llc=(lon_lo, lat_lo), south_pole=pole, hydrometeors=HYDS, seed=7)
    jj, ii = np.meshgrid(np.arange(ny, dtype=np.float32), np.arange(nx, dtype=np.float32), indexing='ij')
    eta = ((nz - np.arange(nz) - 0.5) / nz) ** 1.5
    z = np.broadcast_to((22000.0 * eta).astype(np.float32)[:, None, None], (nz, ny, nx)).copy()
    wave = (1.0 + 0.5 * np.sin(0.7 * jj + 0.3) * np.cos(0.9 * ii + 0.1)).astype(np.float32)[None]
    T = (288.0 - 6.5e-3 * z).astype(np.float32)
    zero = np.zeros_like(z)
    data = {'U': (8.0 + 2.0 * wave + 0 * z).astype(np.float32), 'V': (-3.0 + wave + 0 * z).astype(np.float32), 'W': zero.copy(),
            'QR_v': (1e-3 * wave * (z < 4000.0)).astype(np.float32), 'QS_v': zero.copy(), 'QG_v': zero.copy(), 'QI_v': zero.copy(),
            'RHO': (1.2 * np.exp(-z / 8000.0)).astype(np.float32), 'T': T}
    proj = {'Lo1': lon_lo, 'La1': lat_lo, 'Lo2': lon_lo + dlon * (nx - 1), 'La2': lat_lo + dlat * (ny - 1),
            'Latitude_of_southern_pole': pole[0], 'Longitude_of_southern_pole': pole[1]}
    return dict(data=data, zlevels=z, proj_info=proj, resolution=np.asarray([dlon, dlat], dtype=np.float32))


def pole_for_origin(site):
    """The south pole under which a NORTHERN site lies at the rotated origin: 90 degrees south of it on its meridian."""
    assert 0.0 < site[0] < 90.0
    return (site[0] - 90.0, site[1])


def pole_for_equator(site, pole_lat, rlat):
    """The longitude of a south pole of latitude pole_lat that puts `site` at the rotated latitude rlat (west of the rotated
    origin), by a scan and bisection over the pole's longitude."""
    lon = np.linspace(site[1], site[1] + 180.0, 3601)
    v = rotate64(site[0], site[1], (pole_lat, lon))[0] - rlat
    k = np.nonzero(np.sign(v[1:]) != np.sign(v[:-1]))[0][0]
    lo, hi = lon[k], lon[k + 1]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if np.sign(rotate64(site[0], site[1], (pole_lat, mid))[0] - rlat) == np.sign(v[k]):
            lo = mid
        else:
            hi = mid
    return (pole_lat, float((lo + 180.0) % 360.0 - 180.0))


class Scenario(object):
    def __init__(self, name, conf, cube, az, el, leaves=False, near_pole=False, planted=None):
        """`leaves`: whether gates leave the cube (None: whatever exact_coords says)."""
        self.name, self.conf, self.cube = name, conf, cube
        self.az, self.el = np.asarray(az, np.float64), np.asarray(el, np.float64)
        self.leaves, self.near_pole, self.planted = leaves, near_pole, planted
        self.site = tuple(conf['radar']['coords'])
        p = cube['proj_info']
        self.pole = (p['Latitude_of_southern_pole'], p['Longitude_of_southern_pole'])
        self.proj, self.res = p, cube['resolution']
        self.s_max = s_max_of(conf)
        self.n_gates = len(np.arange(conf['radar']['radial_resolution'] / 2., conf['radar']['range'], conf['radar']['radial_resolution']))
        assert len(self.az) <= 48 and self.n_gates <= 100 and cube['zlevels'].shape[0] <= 12
        # (a sweep with a gate outside the domain raises IndexError once its arrays are complete: the tests expect it exactly here)
        self.leaves = not in_domain(self.exact(), self.proj).all()
        assert leaves is None or leaves == self.leaves

    def with_quadrature(self, nh, nv, n_rays=None):
        """The same scenario under another antenna quadrature (form B: nh = nv = 1), optionally with its first n_rays rays
        (repeated cyclically beyond their number, shifted by 0.37 degrees per round)."""
        conf = copy.deepcopy(self.conf)
        conf['integration'].update(nh_GH=nh, nv_GH=nv)
        az, el = self.az, self.el
        if n_rays is not None:
            k = np.arange(n_rays)
            az, el = (az[k % len(az)] + 0.37 * (k // len(az))) % 360.0, el[k % len(el)]
        return Scenario('%s_%dx%d_%d' % (self.name, nh, nv, len(az)), conf, self.cube, az, el, None, self.near_pole, self.planted)

    def luts(self):
        return _luts()

    def sub(self):
        return quadrature.subbeams(self.conf)

    def fit(self):
        return host_fit(self.site, self.pole, node_azimuths(self.conf, self.az), self.s_max)

    def host_traj(self):
        """float32 arc distances [n_rays, n_v, n_gates] as the device's ray_path forms them (float64 statements of
        atm_refraction.py:206-215, one float32 cast): what the debug read `traj` returns, for the CPU tests."""
        sub = self.sub()
        r = self.conf['radar']
        rr = np.arange(r['radial_resolution'] / 2., r['range'], r['radial_resolution'])
        re, ke = geometry.earth_radius_for_refraction(self.site)
        el = np.deg2rad(sub.pts_ver[None, :] + self.el[:, None])[..., None]
        ke_re = ke * re
        temp = np.sqrt(rr * rr + ke_re * ke_re + 2.0 * rr * ke * re * np.sin(el))
        h = temp - ke_re + self.site[2]
        return (ke_re * np.arcsin((rr * np.cos(el)) / (ke_re + h))).astype(np.float32)

    def exact(self, s32=None):
        sub = self.sub()
        return exact_coords(self.site, self.pole, node_azimuths(self.conf, self.az), self.host_traj() if s32 is None else s32,
                            sub.sub_h, sub.sub_v)


_LUTS = {}


def _luts():
    if 'l' not in _LUTS:
        _LUTS['l'] = synthetic.make_all_luts(TABLES, 5.6, '1mom', n_e=8)
    return _LUTS['l']


def _around(site, pole, half, res, nz=8, shrink=None):
    """A square cube of +-half degrees (rotated) around the site, on a grid aligned to multiples of res."""
    rlat, rlon = rotate64(site[0], site[1], pole)
    h = half if shrink is None else shrink
    la0 = np.floor((rlat - h) / res) * res
    lo0 = np.floor((rlon - h) / res) * res
    return _cube(round(la0, 6), round(la0 + 2 * h + res, 6), round(lo0, 6), round(lo0 + 2 * h + res, 6), res, res, pole, nz)


def _plant(site, pole, s_max, n_gates_s, want_bad, want_rejected, want_sound):
    """Azimuths near the rotated pole chosen by host_fit over 720 candidates: rays that the node rule accepts and whose
    polynomial is more than 2 ulp off somewhere, rays that rule rejects, and sound rays.  -> (az, {class: indices})"""
    cand = np.arange(1440) * 0.25
    f = host_fit(site, pole, cand[:, None], s_max)
    s = np.linspace(0.0, s_max / 1.001, n_gates_s)[None, :].repeat(len(cand), 0)
    ex = exact_at(site, pole, cand[:, None], s)
    err = (np.abs(poly_at(f['coef'], s, s_max)[:, 0] - ex) / ulp32(ex)).max(axis=(1, 2))
    acc = f['sane_nodes'][:, 0]
    # (no candidate at either rule's threshold: the device's sincos may differ from NumPy's in the last bit)
    clear = (np.abs(f['node_step'][:, 0] - RULE_NODE_STEP) > 1e-3) & (np.abs(tail_ratio(f)[:, 0] - 1.0) > 1e-2)

    def spread(idx, n):
        return idx[np.linspace(0, len(idx) - 1, min(n, len(idx))).astype(int)] if len(idx) else idx
    bad = np.nonzero(acc & (err > 2.0) & clear)[0]
    bad = bad[np.argsort(-err[bad])][:want_bad]
    rej = spread(np.nonzero(~acc & clear)[0], want_rejected)
    kept = spread(np.nonzero(f['sane'][:, 0] & clear)[0], want_sound // 2)       # accepted by the tail rule as well
    good = np.concatenate([kept, spread(np.nonzero(acc & ~f['sane'][:, 0] & (err < 0.25) & clear)[0], want_sound - len(kept))])
    idx = np.concatenate([bad, rej, good])
    return cand[idx], {'bad': np.arange(len(bad)), 'rejected': len(bad) + np.arange(len(rej)),
                       'sound': len(bad) + len(rej) + np.arange(len(good))}


def _near_pole(name, dist_deg, rng, step, grid):
    """Site SITE, the rotated north pole dist_deg east of it (the site at a rotated longitude of about -90, away from the wrap);
    `grid` = (rlat_lo, rlat_hi, dlat, dlon): a strip beside the pole over (nearly) all rotated longitudes."""
    np_lat, np_lon = geodesy.wgs84_direct(SITE[0], SITE[1], 90.0, dist_deg * DEG * 6371000.0)
    pole = (-float(np_lat), float(np_lon) - 180.0)
    conf = _conf(SITE, rng, step)
    az, classes = _plant(SITE, pole, s_max_of(conf), 400, 20, 12, 16)
    la0, la1, dlat, dlon = grid
    cube = _cube(la0, la1, -178.0, 178.0, dlat, dlon, pole)
    el = np.full(len(az), 1.5)
    return Scenario(name, conf, cube, az, el, leaves=None, near_pole=True, planted=classes)


NAMES = ['control', 'equator_unrotated', 'southern', 'high_latitude', 'cardinal', 'long_range', 'fine_grid', 'leaves_domain',
         'rlon_wrap', 'near_pole_50km_02', 'near_pole_50km_075', 'near_pole_3deg', 'far_pole_500km']
NEAR_POLE = [n for n in NAMES if 'pole' in n]
_SCN = {}


def scenario(name):
    if name not in _SCN:
        _SCN[name] = _build(name)
    return _SCN[name]


def _build(name):
    az48 = 1.3 + 7.5 * np.arange(48)
    el48 = np.tile([0.5, 1.5, 4.0, 9.0], 12)
    if name == 'control':
        conf = _conf(SITE, 50000, 500)
        return Scenario(name, conf, _around(SITE, POLE, 0.55, 0.02), az48, el48)
    if name == 'equator_unrotated':
        site, pole = (0.0, 0.0, 1000.0), (-90.0, 0.0)
        return Scenario(name, _conf(site, 50000, 500), _around(site, pole, 0.55, 0.02), az48, el48)
    if name == 'southern':
        site = (-33.0, 151.0, 100.0)
        # (a rotation without a third angle has its origin at 90 - |pole latitude| NORTH: no pole puts a southern site there.  The
        # nearest thing: the site beside the rotated EQUATOR, which under a pole at 30 S reaches 60 S)
        pole = pole_for_equator(site, -30.0, 0.31)
        return Scenario(name, _conf(site, 50000, 500), _around(site, pole, 0.55, 0.02), az48, el48)
    if name == 'high_latitude':
        site = (78.0, 15.0, 100.0)
        pole = pole_for_origin(site)                        # (-12, 15): the rotated north pole at 12 N 165 W
        return Scenario(name, _conf(site, 50000, 500), _around(site, pole, 0.55, 0.02), az48, el48)
    if name == 'cardinal':
        az = []
        for c in (0.0, 90.0, 180.0, 270.0):
            az += [np.nextafter(c, -1.0) % 360.0 if c else np.nextafter(360.0, 0.0), c, np.nextafter(c, 400.0)]
        az = np.repeat(np.asarray(az), 4)
        el = np.tile([0.5, 45.0, 89.0, 90.0], 12)
        return Scenario(name, _conf(SITE, 50000, 500), _around(SITE, POLE, 0.55, 0.02), az, el)
    if name == 'long_range':
        return Scenario(name, _conf(SITE, 500000, 5000), _around(SITE, POLE, 5.2, 0.1), az48, el48)
    if name == 'fine_grid':
        # rotated coordinates of several degrees: a float32 ulp there is 4.8e-7 deg, 1 / 4000 of a 0.002-deg cell
        lat, lon = geodesy.rotated_to_wgs(5.3, 6.9, POLE[0], POLE[1])
        site = (float(lat), float(lon), 500.0)
        return Scenario(name, _conf(site, 20000, 200), _around(site, POLE, 0.25, 0.002), az48, el48)
    if name == 'leaves_domain':
        return Scenario(name, _conf(SITE, 50000, 500), _around(SITE, POLE, 0.55, 0.02, shrink=0.25), az48, el48, leaves=True)
    if name == 'rlon_wrap':
        lat, lon = geodesy.rotated_to_wgs(0.3, 179.6, POLE[0], POLE[1])
        site = (float(lat), float(lon), 500.0)
        conf = _conf(site, 50000, 500, nh=3, nv=3)
        cube = _cube(-0.3, 0.9, 178.9, 179.9, 0.02, 0.02, POLE)
        # eastward rays cross +-180 (and leave the domain): some between two nodes (the node rule's 360-degree jump), and -- searched
        # here -- some between the last node, x = cos(pi / 18), and the last gate: an accepted fit extrapolated over the wrap
        s_max = s_max_of(conf)
        cand = np.arange(30.0, 150.0, 0.01)
        last_node = exact_at(site, POLE, cand, (NODES[0] + 1.0) * s_max / 2.0)[..., 1]
        last_gate = exact_at(site, POLE, cand, s_max / 1.001 * np.cos(np.deg2rad(1.5)))[..., 1]
        late = cand[(last_node > 0) & (last_gate < 0)]
        assert len(late) >= 2, len(late)
        az = np.concatenate([late[[0, len(late) // 2, -1]], 40.0 + 5.0 * np.arange(21), 181.3 + 7.5 * np.arange(24)])
        return Scenario(name, conf, cube, az, np.full(len(az), 1.5), leaves=True)
    if name == 'near_pole_50km_02':
        return _near_pole(name, 0.2, 50000, 500, (89.3, 89.98, 0.02, 2.0))
    if name == 'near_pole_50km_075':
        return _near_pole(name, 0.75, 50000, 500, (88.7, 89.9, 0.02, 2.0))
    if name == 'near_pole_3deg':
        return _near_pole(name, 3.0, 150000, 1500, (85.5, 88.5, 0.05, 1.0))
    if name == 'far_pole_500km':
        return _near_pole(name, 6.0, 500000, 5000, (79.0, 89.0, 0.1, 1.0))
    raise KeyError(name)
