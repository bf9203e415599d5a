"""k_ml_weights (cosmo_pol_amd/csrc/cpol_final.inl) -- the per-gate sub-beam weights of integration scheme 'ml' -- at gate counts
below, at and beyond the filter radius and the wavefront, with the melting layer at every place along the ray, through sweeps
(simulate_rays with the debug reads on: sub_wgate) and through the sub-beam export (interpolate_rays: quad_weights) on a small,
horizontally uniform synthetic cube: flat levels 400 m apart, rain up to one height, snow and graupel from a lower height on,
and in one variant a slab without snow and graupel, so that the layer has two separate segments.

The reference: for the sub-beams with sub_smooth, sub_w x scipy.ndimage.gaussian_filter(deltas, 2) with `deltas` 1.0 at the first
and at the last gate of the float32 mask QR > 0 and QS + QG > 0 of the EXPORTED columns (the values before the melting scheme) and
0.0 elsewhere -- all zeros where the mask is empty or the configuration does not melt; for the other sub-beams sub_w x 1.
Compared BIT FOR BIT: the kernel's tap order -- the centre tap, then pairs from the outermost tap inwards, 'reflect' applied
repeatedly where a tap leaves a ray shorter than the radius of 8 -- is scipy's (that order restated in Python gave scipy's bits
on 1 490 patterns of two deltas: every pair of gates at 1 to 19 gates, pairs at and next to both ends at 63, 64, 65 and 129).
The coverage -- the layer at gate 0, reaching the last gate, of one gate, absent, wholly beyond gate 64, straddling gate 64, in two segments -- is asserted from the exported columns.

All 39 tests pass on the library as it is.  Tried against a scratch build with reflect_index applied once (`if` for `while`; the
index is only compared, never used as an address): 8 fail -- test_weights_are_scipys_bits at 1, 2 and 5 gates (scenes 'inside'
and 'steep', both horizontal node counts), the rays shorter than the filter radius of 8, where a tap has to be reflected more
than once; 8 gates and more pass, as they must.  The five edits of k_ice_first and gate_finish are recorded in
tests/test_gpu_rvel.py."""
import copy
import functools

import numpy as np
import pytest

import _cases
import _scans
from cosmo_pol_amd import quadrature, synthetic

pytestmark = pytest.mark.gpu

KNOBS = ('CPOL_GATE1', 'CPOL_GATE1_RAY', 'CPOL_FUSE_CLASSIFY', 'CPOL_RARE_DIRECT', 'CPOL_SUBSUM', 'CPOL_USE_GRAPH', 'CPOL_EXP_SKIP', 'CPOL_ITAB')
LEVEL_STEP = 400.0                                       # m between the flat model levels (31 of them: 12 000 m ... 0 m)
RAIN_TOP, SNOW_BASE, GRAUPEL_BASE = 2400.0, 1600.0, 2000.0         # the highest level with rain, the lowest with snow / graupel
SLAB = (2000.0, 2400.0)                                  # variant 'slab': no snow and no graupel on these two levels
RADIUS = 8                                               # taps on either side of scipy's gaussian_filter(., 2)
AZIMUTHS = (30.0, 200.0)
# name: (site altitude m, elevation deg, {gate count: radial resolution m}, cube variant): the configuration takes ranges from 5 km
# on, so the short rays have long gates.  The layer lies where the interpolated QR and QS + QG are both positive: heights between
# 1200 m and 2800 m (variant 'slab': without 2000 m ... 2400 m)
SCENES = {
    'inside':   (2000, 5.0, {1: 5000, 2: 2500, 5: 1000, 8: 625, 9: 600, 17: 300}, 'plain'),       # the site inside the layer: gate 0 to the last gate
    'climb':    (500, 10.0, {63: 150, 64: 150, 65: 150, 129: 150}, 'plain'),                       # entered near gate 27, left near gate 88
    'late':     (500, 2.5, {65: 200, 129: 200}, 'plain'),                                          # entered beyond gate 64 (65 gates: never)
    'steep':    (500, 60.0, {5: 1500}, 'plain'),                                                   # one gate inside
    'above':    (3000, 5.0, {9: 600}, 'plain'),                                                    # never
    'segments': (500, 10.0, {129: 150}, 'slab'),
    'leaving':  (2100, 20.0, {17: 300}, 'slab'),                                                   # the site inside the slab: the layer begins a few gates out
}
RUNS = [(name, n) for name, sc in SCENES.items() for n in sc[2]]


@functools.lru_cache(maxsize=None)
def cube(variant):
    c = synthetic.small_test_cube(hydrometeors=('R', 'S', 'G'), **dict(_cases.gen_golden.CUBE_KW, nz=31))
    nz, ny, nx = c['zlevels'].shape
    z = (LEVEL_STEP * np.arange(nz - 1, -1, -1)).astype(np.float32)
    c['zlevels'] = np.ascontiguousarray(np.broadcast_to(z[:, None, None], (nz, ny, nx)))
    col = {'QR_v': np.where(z <= RAIN_TOP, 1.0e-3, 0.0), 'QS_v': np.where(z >= SNOW_BASE, 5.0e-4, 0.0),
           'QG_v': np.where(z >= GRAUPEL_BASE, 2.0e-4, 0.0), 'QI_v': np.zeros(nz), 'T': 288.0 - 6.5e-3 * z,
           'RHO': 1.2 * np.exp(-z / 8000.0), 'U': 8.0 + 6e-4 * z, 'V': -3.0 + 2e-4 * z, 'W': np.zeros(nz)}
    if variant == 'slab':
        for k in ('QS_v', 'QG_v'):
            col[k] = np.where((z >= SLAB[0]) & (z <= SLAB[1]), 0.0, col[k])
    for k, v in col.items():
        assert k in c['data'], k
        c['data'][k] = np.ascontiguousarray(np.broadcast_to(v.astype(np.float32)[:, None, None], (nz, ny, nx)))
    return c


def overrides(nh, melting, scene, n_gates):
    alt, el, res, _ = SCENES[scene]
    res = res[n_gates]
    over = copy.deepcopy(_cases.gen_golden.radial_case_inputs('q_ml')[0])
    over['radar'].update(coords=[46.5, 7.5, alt], radial_resolution=int(res), range=int(res * n_gates))
    over['microphysics'].update(with_melting=int(melting), with_ice_crystals=0)
    over['integration'] = {'scheme': 'ml', 'nh_GH': int(nh), 'nv_GH': 1, 'weight_threshold': 1.}
    return over


class Operators(object):
    """One operator per (nh_GH, melting); the scene goes in through its configuration, the cube is loaded when it changes."""

    def __init__(self):
        self.ops, self.loaded = {}, {}

    def get(self, nh, melting, scene, n_gates):
        from cosmo_pol_amd import RadarOperator
        over = overrides(nh, melting, scene, n_gates)
        key = (nh, melting)
        if key not in self.ops:
            conf = _cases.radial_case('q_ml')[0]
            luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in ('R', 'S', 'G', 'mS', 'mG')}
            luts = {h: l for h, l in luts.items() if melting or h not in ('mS', 'mG')}
            with pytest.MonkeyPatch.context() as mp:
                for k in KNOBS:
                    mp.delenv(k, raising=False)
                self.ops[key] = RadarOperator(config=over, luts=luts, output_variables='only_radar')
        op = self.ops[key]
        conf = op.config
        for sec, d in over.items():
            conf[sec].update(copy.deepcopy(d))
        op.config = conf
        got = op.config
        assert got['radar']['coords'][2] == SCENES[scene][0] and got['radar']['radial_resolution'] == SCENES[scene][2][n_gates] and \
            got['radar']['range'] == SCENES[scene][2][n_gates] * n_gates and \
            got['integration']['scheme'] == 'ml' and got['integration']['nh_GH'] == nh and got['microphysics']['with_melting'] == melting, got
        variant = SCENES[scene][3]
        if self.loaded.get(key) != variant:
            c = cube(variant)
            op.load_model_arrays(c['data'], c['zlevels'], c['proj_info'], c['resolution'])
            self.loaded[key] = variant
        return op

    def close(self):
        for op in self.ops.values():
            op.close()
        self.ops = {}


@pytest.fixture(scope='module')
def operators():
    o = Operators()
    yield o
    o.close()


def layer_mask(cols):
    """bool [n_rays, n_sub, n_gates]: melting.py:41 on the exported float32 values."""
    qr, qs, qg = (np.asarray(cols[k]) for k in ('QR_v', 'QS_v', 'QG_v'))
    assert qr.dtype == qs.dtype == qg.dtype == np.float32
    with np.errstate(invalid='ignore'):
        return (qr > 0) & ((qs + qg) > 0)


def reference(mask, sub_w, sub_smooth, melting):
    from scipy.ndimage import gaussian_filter
    out = np.empty(mask.shape, dtype=np.float64)
    for r in range(mask.shape[0]):
        for s in range(mask.shape[1]):
            if not sub_smooth[s]:
                out[r, s] = sub_w[s] * 1.0
                continue
            deltas = np.zeros(mask.shape[2])
            w = np.flatnonzero(mask[r, s])
            if melting and len(w):
                deltas[w[0]] = deltas[w[-1]] = 1.0
            out[r, s] = sub_w[s] * gaussian_filter(deltas, 2)
    return out


def coverage_of(mask, sub_smooth):
    """What the layer mask of one export shows, over its smoothed sub-beams."""
    seen = set()
    n = mask.shape[2]
    for r in range(mask.shape[0]):
        for s in np.flatnonzero(sub_smooth):
            w = np.flatnonzero(mask[r, s])
            if not len(w):
                seen.add('no_layer')
                continue
            if w[0] == 0:
                seen.add('at_gate_0')
            if w[-1] == n - 1:
                seen.add('reaches_last_gate')
            if len(w) == 1 and n > 1:
                seen.add('one_gate')
            if w[0] > 64:
                seen.add('wholly_beyond_64')
            if w[0] < 64 < w[-1]:
                seen.add('straddles_64')
            if len(w) < w[-1] - w[0] + 1:
                seen.add('two_segments')
            if n <= RADIUS:
                seen.add('shorter_than_radius')
            if 0 < w[0] < RADIUS or 0 < n - 1 - w[-1] < RADIUS:
                seen.add('reflected_at_an_end')
    return seen


@pytest.fixture(scope='module')
def seen(operators):
    """(scene, n_gates, nh) -> coverage_of the columns exported for it: the exports are made here, so the coverage test stands
    alone."""
    out = {}
    for nh in (1, 3):
        for scene, n_gates in RUNS:
            op = operators.get(nh, 1, scene, n_gates)
            az, el = np.array(AZIMUTHS), np.full(len(AZIMUTHS), SCENES[scene][1])
            cols = op.interpolate_rays(az, el, melting=False)
            out[(scene, n_gates, nh)] = coverage_of(layer_mask(cols), quadrature.subbeams(op.config).sub_smooth)
    return out


@pytest.mark.parametrize('nh', (1, 3))
@pytest.mark.parametrize('scene,n_gates', RUNS, ids=['%s_g%d' % r for r in RUNS])
def test_weights_are_scipys_bits(operators, scene, n_gates, nh):
    """Melting on: the sweep's sub_wgate and the export's quad_weights against the reference on the exported columns."""
    op = operators.get(nh, 1, scene, n_gates)
    az, el = np.array(AZIMUTHS), np.full(len(AZIMUTHS), SCENES[scene][1])
    sub = quadrature.subbeams(op.config)
    assert sub.n_sub == 11 * nh and sub.sub_smooth.sum() > 0 and (sub.sub_smooth == 0).sum() > 0 and sub.ml_radius == RADIUS
    cols = op.interpolate_rays(az, el, melting=False)
    assert cols['QR_v'].shape == (2, sub.n_sub, n_gates)
    mask = layer_mask(cols)
    want = reference(mask, sub.sub_w, sub.sub_smooth, True)
    assert _scans.same_bits(np.asarray(cols['quad_weights']), want), (scene, n_gates, _scans.where_differs(np.asarray(cols['quad_weights']), want))
    melted = op.interpolate_rays(az, el, melting=True)
    assert _scans.same_bits(np.asarray(melted['quad_weights']), want)
    ctx = op._lane(0)
    ctx.enable_debug(True)
    try:
        res = op.simulate_rays(az, el)
        got = ctx.debug_read('sub_wgate', (2, sub.n_sub, n_gates), np.float64)
    finally:
        ctx.enable_debug(False)
    assert res['ZH'].shape == (2, n_gates)
    assert _scans.same_bits(got, want), (scene, n_gates, _scans.where_differs(got, want))


@pytest.mark.parametrize('nh', (1, 3))
@pytest.mark.parametrize('scene,n_gates', [('inside', 5), ('climb', 129), ('segments', 129)])
def test_without_melting_the_smoothed_sub_beams_weigh_nothing(operators, scene, n_gates, nh):
    op = operators.get(nh, 0, scene, n_gates)
    az, el = np.array(AZIMUTHS), np.full(len(AZIMUTHS), SCENES[scene][1])
    sub = quadrature.subbeams(op.config)
    cols = op.interpolate_rays(az, el, melting=False)
    assert layer_mask(cols).any()
    want = reference(layer_mask(cols), sub.sub_w, sub.sub_smooth, False)
    assert (want[:, sub.sub_smooth != 0] == 0).all() and (want[:, sub.sub_smooth == 0] > 0).all()
    ctx = op._lane(0)
    ctx.enable_debug(True)
    try:
        op.simulate_rays(az, el)
        got = ctx.debug_read('sub_wgate', (2, sub.n_sub, n_gates), np.float64)
    finally:
        ctx.enable_debug(False)
    assert _scans.same_bits(got, want) and _scans.same_bits(np.asarray(cols['quad_weights']), want)


def test_scenes_cover_what_they_claim(seen):
    """From the exported columns of every scene (the fixture's own exports)."""
    SEEN = seen
    assert len(SEEN) == 2 * len(RUNS)
    seen = set().union(*SEEN.values())
    need = {'no_layer', 'at_gate_0', 'reaches_last_gate', 'one_gate', 'wholly_beyond_64', 'straddles_64', 'two_segments',
            'shorter_than_radius', 'reflected_at_an_end'}
    assert need <= seen, sorted(need - seen)
    assert {n for _, n, _ in SEEN} == {1, 2, 5, 8, 9, 17, 63, 64, 65, 129}
    for scene, want in (('inside', {'at_gate_0', 'reaches_last_gate'}), ('late', {'wholly_beyond_64'}), ('steep', {'one_gate'}),
                        ('above', {'no_layer'}), ('segments', {'two_segments'}), ('climb', {'straddles_64'})):
        got = set().union(*[v for k, v in SEEN.items() if k[0] == scene])
        assert want <= got, (scene, sorted(got))
