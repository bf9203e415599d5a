"""Terrain shadowing on the GPU (cpol_sweep_params.terrain_shadow, cpol_outputs.visibility; k_terrain_shadow, k_visibility):
the kernel alone against the rule in NumPy, the seam identity -- a shadowing operator's sweep against its own column call on the
unshadowed export shadowed on the host -- the stencil life cycle, the ensemble / timed / composite identities under shadowing, the
visibility array, the refusals, and the keys left off.

THE TERRAIN.  synthetic.small_test_cube() with its z-levels rebuilt by make_cube's hybrid formula over a topography capped at 900 m
plus one ridge: an arc 20 km from the radar (which stands at 1000 m), 2 km wide (Gaussian), crest 1950 m, over the azimuths 60 .. 120
degrees.  Twelve rays: azimuths 30, 60, 75, 90, 105, 150 at elevations 1 and 3 degrees, 170 gates of 300 m.  At 1 degree the beam
centre passes the ridge at ~1370 m and the node 0.57 degrees above it at ~1570 m: every sub-beam is blocked, and valid gates
follow behind the ridge.  At 3 degrees the centre passes at ~2070 m and only the lower nodes (0.52 / 0.57 degrees lower: ~1890 /
~1870 m) are blocked: partial visibility.  The rays at 30 and 150 degrees meet no terrain.  Checked with the oracle's beam and
interpolation on the CPU before the first GPU run; every test asserts what it needs of this from the unshadowed export."""
import copy
import functools

import numpy as np
import pytest

import _cases
import gen_golden as GG
from cosmo_pol_oracle import config as ocfg

pytestmark = pytest.mark.gpu

MODEL_TOP = 22000.0                 # make_cube's default
AZ = np.repeat([30.0, 60.0, 75.0, 90.0, 105.0, 150.0], 2)
EL = np.tile([1.0, 3.0], 6)
FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL', 'mask']
GEOM = ['lats', 'lons', 'dist', 'heights']
RSG, RSGI = ('R', 'S', 'G'), ('R', 'S', 'G', 'I')
#         integration                                             microphysics                                   doppler  cube  2mom  frequency
CASES = {
    'one':      ({'nh_GH': 1, 'nv_GH': 1},                          {'with_ice_crystals': 0, 'with_melting': 0}, 1, RSG, False, 5.6),
    '3x3':      ({'nh_GH': 3, 'nv_GH': 3, 'weight_threshold': 1.},  {'with_ice_crystals': 0, 'with_melting': 0}, 1, RSG, False, 5.6),
    '7x7':      ({'nh_GH': 7, 'nv_GH': 7, 'weight_threshold': 1.},  {'with_ice_crystals': 0, 'with_melting': 0}, 0, RSG, False, 5.6),
    'melt_ice': ({'nh_GH': 1, 'nv_GH': 3, 'weight_threshold': 1.},  {'with_ice_crystals': 1, 'with_melting': 1}, 1, RSGI, False, 5.6),
    '2mom':     ({'nh_GH': 1, 'nv_GH': 3, 'weight_threshold': 1.},
                 {'scheme': '2mom', 'with_ice_crystals': 1, 'with_melting': 0}, 1, RSGI, True, 13.6),
    'dop2':     ({'nh_GH': 3, 'nv_GH': 3, 'weight_threshold': 1.},  {'with_ice_crystals': 1, 'with_melting': 1}, 2, RSGI, False, 5.6),
    # scheme 'ml' without the melting scheme: the per-gate weights do not read the values (cpol_final.inl: k_ml_weights), so
    # the unshadowed export's weights are the shadowing sweep's and the identity holds as it stands
    'ml':       ({'scheme': 'ml', 'nh_GH': 3, 'nv_GH': 3, 'weight_threshold': 0.9999},
                 {'with_ice_crystals': 0, 'with_melting': 0}, 1, RSG, False, 5.6),
    # ... with it the weights are made from the first and the last melting gate of the SHADOWED sub-beam (the step runs before
    # the 'ml' weights): the column call then takes the shadowing operator's own exported weights, everything else from A
    'ml_melt':  ({'scheme': 'ml', 'nh_GH': 3, 'nv_GH': 3, 'weight_threshold': 0.9999},
                 {'with_ice_crystals': 1, 'with_melting': 1}, 1, RSGI, False, 5.6),
}
ON = {'terrain_shadow': 1, 'terrain_visibility': 1}


def shadow_mod():
    from cosmo_pol_amd import shadow
    return shadow


def ridge_cube(cube, r_km=20.0, width_km=2.0, crest=1950.0, sector=(60.0, 120.0), base_cap=900.0):
    """The cube over a topography capped at `base_cap` with one ridge; z-levels by make_cube's hybrid formula."""
    z = cube['zlevels']
    nz, ny, nx = z.shape
    eta = ((nz - np.arange(nz) - 0.5) / nz).astype(np.float64) ** 1.5
    e_last = float(np.float32(eta[-1]))
    topo = np.minimum((z[-1].astype(np.float64) - MODEL_TOP * e_last) / (1.0 - e_last), base_cap)       # (the lowest level, inverted)
    km = float(cube['resolution'][0]) * 111.2
    jy, jx = np.mgrid[0:ny, 0:nx]
    dy, dx = (jy - ny // 2) * km, (jx - nx // 2) * km        # (the radar stands at the centre of the cube)
    r, az = np.hypot(dx, dy), np.degrees(np.arctan2(dx, dy)) % 360.0
    ridge = np.where((az >= sector[0]) & (az <= sector[1]), crest * np.exp(-((r - r_km) / width_km) ** 2 / 2.0), 0.0)
    topo = np.maximum(topo, ridge).astype(np.float32)
    znew = (topo[None] + (np.float32(MODEL_TOP) - topo)[None] * eta.astype(np.float32)[:, None, None]).astype(np.float32)
    return dict(cube, zlevels=znew)


@functools.lru_cache(maxsize=None)
def cube_for(hyds, two):
    from cosmo_pol_amd import synthetic
    return ridge_cube(synthetic.small_test_cube(hydrometeors=hyds, two_moment=two, **GG.CUBE_KW))


def config_for(name, extra=None):
    integ, micro, dop, hyds, two, freq = CASES[name]
    conf = {'radar': {'coords': [46.5, 7.5, 1000], 'frequency': freq, '3dB_beamwidth': 1., 'K_squared': 0.93, 'type': 'ground',
                      'sensitivity': [-5, 10000], 'range': 51000, 'radial_resolution': 300},
            'doppler': {'scheme': dop if dop else 1}, 'microphysics': dict(micro), 'integration': dict(integ)}
    luts_conf = ocfg.make_config(copy.deepcopy(conf))
    luts = {h: _cases.synthetic_lut(h, freq, luts_conf['microphysics']['scheme']) for h in ocfg.hydrometeor_list(luts_conf)}
    if extra:
        conf['integration'].update(extra)
    return conf, luts, cube_for(hyds, two)


def operator(name, extra=None, cube=None, **kw):
    from cosmo_pol_amd import RadarOperator
    conf, luts, c = config_for(name, extra)
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar', **kw)
    c = cube or c
    op.load_model_arrays(c['data'], c['zlevels'], c['proj_info'], c['resolution'])
    return op


def arrays(res):
    return {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}


def same_bits(a, b):
    """dtype, shape and every element: equal bits, or NaN on both sides"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return a.tobytes() == b.tobytes()
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.ascontiguousarray(a)[~na].view(u), np.ascontiguousarray(b)[~nb].view(u)))


def preconditions(cols, n_sub):
    """What the terrain must give, read off the UNSHADOWED export: -> (rays fully blocked behind a hit that valid gates follow,
    gates of partial visibility, rays without any -1)."""
    S = shadow_mod()
    mask = np.asarray(cols['mask'])
    n_rays, _, ng = mask.shape
    first = S.first_hit(mask)
    behind = np.array([[(mask[r, s, first[r, s]:] == 0).sum() if first[r, s] < ng else 0 for s in range(n_sub)] for r in range(n_rays)])
    full = np.where(((first < ng) & (behind > 0)).all(axis=1))[0]
    untouched = np.where(~(mask == -1).any(axis=(1, 2)))[0]
    assert len(full) >= 1, 'no ray fully blocked behind a hit that is followed by valid gates'
    assert len(untouched) >= 1, 'no ray without a gate below the topography'
    partial = np.zeros((n_rays, ng), dtype=bool)
    w = np.asarray(cols['quad_weights'])
    if n_sub > 1 and w.ndim == 1:
        v0, v1 = S.visibility(mask, w), S.visibility(S.apply(strip(cols))['mask'], w)
        partial = (v1 > 0) & (v1 < 1) & (v0 == 1.0)
        assert partial.any(), 'no gate with 0 < visibility < 1 whose unshadowed visibility is 1'
    return full, partial, untouched


def strip(cols):
    """the columns of an export without what a column call on raw values does not take"""
    return {k: v for k, v in cols.items() if k not in ('QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG', 'mask_ml', 'has_melting')}


# ------------------------------------------------------------------ 1. the kernel alone
def _rows(n_gates, rng):
    """Rows with the first hit at: none, 0, 1, 62, 63, 64, 65, n_gates - 1 (where the row is that long), each with further hits and +1 / 2
    codes on either side of it."""
    rows = []
    for first in [None, 0, 1, 62, 63, 64, 65, n_gates - 1]:
        if first is not None and not 0 <= first < n_gates:
            continue
        for variant in range(3):
            c = np.zeros(n_gates, dtype=np.int8)
            if variant:
                c[rng.random(n_gates) < 0.3] = 1
                c[rng.random(n_gates) < 0.1] = 2
            if first is not None:
                if variant == 2:
                    c[first:][rng.random(n_gates - first) < 0.4] = -1      # further hits behind the first
                c[first] = -1
            rows.append(c)
    return np.stack(rows)


@pytest.mark.parametrize('n_vars', [1, 9])
@pytest.mark.parametrize('n_gates', [1, 17, 63, 64, 65, 128, 167, 500])
def test_kernel_alone_equals_the_rule(n_gates, n_vars):
    from cosmo_pol_amd import _native as N
    S = shadow_mod()
    rng = np.random.default_rng(1000 * n_gates + n_vars)
    mask = _rows(n_gates, rng)
    assert len(mask) > 4 or n_gates == 1                    # (more than one workgroup of four rows)
    vals = rng.normal(size=(n_vars,) + mask.shape).astype(np.float32)
    vals[rng.random(vals.shape) < 0.1] = -9999.0
    vals[rng.random(vals.shape) < 0.1] = np.nan
    vals[:, mask == -1] = np.nan                            # (as the interpolation leaves a gate below the topography)
    vals[0, 0, 0] = np.float32(1.5)                         # ... and finite values under a hit and behind it are overwritten all the same
    want_m, want_v = S.apply_arrays(mask, vals)
    ctx = N.Context(0)
    got_m, got_v = ctx.debug_shadow(mask, vals)
    again_m, again_v = ctx.debug_shadow(got_m, got_v)
    ctx.close()
    assert got_m.dtype == np.int8 and got_m.tobytes() == want_m.tobytes()
    hit = S.hit(mask)
    assert np.isnan(got_v[:, hit]).all() and np.isnan(want_v[:, hit]).all()
    assert got_v[:, ~hit].view(np.uint32).tobytes() == vals[:, ~hit].view(np.uint32).tobytes()       # outside the shadow: the caller's bits
    assert again_m.tobytes() == got_m.tobytes() and same_bits(again_v, got_v)                        # idempotent
    first = S.first_hit(mask)
    assert (first == n_gates).any() and (first < n_gates).any()           # (rows without a hit and rows with one)
    assert n_gates == 1 or mask.tobytes() != want_m.tobytes()             # (and the rule moved something)


# ------------------------------------------------------------------ 2. the seam identity
@pytest.mark.parametrize('name', list(CASES))
def test_seam_identity(name):
    """B (shadowing on) against A (off), everything else the same: B's sweep == B's column call on shadow.apply(A's raw export) in
    every output array, B's raw export == shadow.apply(A's), bit for bit.  Gates finite in A's sweep and NaN in B's exist; with more
    than one sub-beam so do gates finite in both with another ZH (partial blocking: the weights are not renormalised) -- with one
    sub-beam everything behind the hit is NaN and no such gate can exist."""
    S = shadow_mod()
    # (the visibility is not defined under scheme 'ml': that key stays off there)
    A, B = operator(name), operator(name, ON if CASES[name][0].get('scheme') != 'ml' else {'terrain_shadow': 1})
    try:
        n_sub = A.simulate_rays(AZ[:1], EL[:1], apply_sensitivity=False)['n_sub']
        a = arrays(A.simulate_rays(AZ, EL, apply_sensitivity=False))
        assert 'visibility' not in a
        cols_a = A.interpolate_rays(AZ, EL, melting=False)
        full, partial, untouched = preconditions(cols_a, n_sub)
        ref = B.simulate_rays(AZ, EL, apply_sensitivity=False)
        forms = B._ctx.launch_forms()
        assert forms['interp_classify'] == 0 and forms['graph_replayed'] == 0
        ref = arrays(ref)
        want_cols = S.apply(strip(cols_a))
        cols_b = B.interpolate_rays(AZ, EL, melting=False)
        assert set(cols_b) == set(want_cols)
        ml = np.asarray(cols_a['quad_weights']).ndim == 3
        for k, v in want_cols.items():
            if k == 'quad_weights' and ml and CASES[name][1]['with_melting']:
                continue                                    # (made from the shadowed values: see CASES)
            assert same_bits(cols_b[k], v), (name, 'export', k)
        if ml and CASES[name][1]['with_melting']:
            assert not same_bits(cols_b['quad_weights'], cols_a['quad_weights'])       # (the case is what it claims to be)
            want_cols = dict(want_cols, quad_weights=cols_b['quad_weights'])
        got = arrays(B.simulate_columns(want_cols))
        assert set(ref) == set(got), set(ref) ^ set(got)
        for k, v in ref.items():
            assert got[k].dtype == v.dtype and got[k].shape == v.shape, (name, k)
            same = (got[k] == v) | (np.isnan(got[k]) & np.isnan(v))
            print('%s %s: %d of %d gates differ' % (name, k, int((~same).sum()), same.size))
            assert np.array_equal(got[k], v, equal_nan=True), (name, k)
        # the feature does something: this fails on a library without it
        lost = np.isfinite(a['ZH']) & np.isnan(ref['ZH'])
        assert lost.any() and lost[full].any() and not lost[untouched].any()
        both = np.isfinite(a['ZH']) & np.isfinite(ref['ZH'])
        if n_sub > 1 and not ml:
            dimmer = both & (a['ZH'] != ref['ZH'])
            assert dimmer.any() and (ref['ZH'][dimmer & partial] < a['ZH'][dimmer & partial]).all() and (dimmer & partial).any()
        for k in FIELDS:
            if k in a:
                assert same_bits(ref[k][untouched], a[k][untouched]), (name, 'untouched rays', k)
        for k in GEOM:                                       # the geometry is never touched
            assert same_bits(ref[k], a[k]), (name, k)
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------ 3. the stencil life cycle under shadowing
def test_identical_sweeps_under_a_version_tag_reach_replay():
    """Five identical single-beam sweeps: the first fetches the gate coordinates of its table set (the long form), the others run
    under the version tag alone -- noted, recorded, replayed, replayed.  Every sweep equals the first, shadow and visibility included."""
    op = operator('one', ON)
    try:
        seen, forms = [], []
        for _ in range(5):
            seen.append(arrays(op.simulate_rays(AZ, EL)))
            forms.append(op.stencil_state()['form'])
            assert op._ctx.launch_forms()['interp_classify'] == 0
        assert forms == [0, 0, 1, 2, 2], forms               # full (twice), recording, replay, replay
        for k in range(1, 5):
            assert set(seen[k]) == set(seen[0])
            for name, v in seen[0].items():
                assert same_bits(seen[k][name], v), (k, name)
        zh, vis = seen[0]['ZH'], seen[0]['visibility']
        assert np.isfinite(zh).any() and np.isnan(zh).any() and (vis == 0.0).any() and (vis == 1.0).any()
    finally:
        op.close()


# ------------------------------------------------------------------ 4. existing identities under shadowing
def other_state(cube):
    data = {k: ((v * np.float32(0.6)).astype(np.float32) if k.startswith('Q') else v) for k, v in cube['data'].items()}
    data['T'] = (cube['data']['T'] - np.float32(3.0)).astype(np.float32)
    # a NaN in variable 0 of this state alone, in a ring the untouched rays cross: this member's codes differ from the other's
    u = data['U'].copy()
    ny, nx = u.shape[1:]
    jy, jx = np.mgrid[0:ny, 0:nx]
    r = np.hypot(jy - ny // 2, jx - nx // 2)
    u[:, (r >= 4.0) & (r < 5.0)] = np.nan
    data['U'] = u
    return dict(cube, data=data)


@pytest.mark.parametrize('name', ['3x3', 'melt_ice'])
def test_every_member_equals_its_own_sweep(name):
    from cosmo_pol_amd import RadarOperator
    conf, luts, cube = config_for(name, ON)
    cubes = [cube, other_state(cube)]
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    try:
        op.load_model_ensemble([c['data'] for c in cubes], cube['zlevels'], cube['proj_info'], cube['resolution'])
        got = arrays(op.simulate_rays_ensemble(AZ, EL, form='shared'))
        assert op._ctx.launch_forms()['interp_classify'] == 0
        assert got['visibility'].shape == (len(AZ), len(op.constants.RANGE_RADAR))
        for m in range(2):
            op.select_member(m)
            ref = arrays(op.simulate_rays(AZ, EL))
            for k in FIELDS:
                if k in ref:
                    assert same_bits(got[k][m], ref[k]), (name, m, k)
            for k in GEOM:
                assert same_bits(got[k], ref[k]), (name, m, k)
            if m == 0:
                assert same_bits(got['visibility'], ref['visibility'])          # (the codes of the call's first member)
        assert not same_bits(got['mask'][0], got['mask'][1])
        assert (np.isnan(got['ZH'][1]) & np.isfinite(got['ZH'][0])).any()        # the ring of NaN shadows member 1 alone
    finally:
        op.close()


def test_timed_sweep_at_the_time_of_a_state_equals_that_states_sweep():
    from cosmo_pol_amd import RadarOperator
    conf, luts, cube = config_for('3x3', ON)
    cubes = [cube, other_state(cube)]
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
    try:
        op.load_model_series([c['data'] for c in cubes], [0.0, 600.0], cube['zlevels'], cube['proj_info'], cube['resolution'])
        for m, t in enumerate([0.0, 600.0]):
            got = arrays(op.simulate_rays_at(AZ, EL, t))
            assert op._ctx.launch_forms()['interp_classify'] == 0
            alone = operator('3x3', ON, cube=cubes[m])
            ref = arrays(alone.simulate_rays(AZ, EL))
            alone.close()
            for k in FIELDS + GEOM + ['visibility']:
                if k in ref:
                    assert same_bits(got[k], ref[k]), (m, k)
            assert (got['visibility'] == 0.0).any() and (got['visibility'] == 1.0).any()
    finally:
        op.close()


def test_composite_maps_equal_the_rule_on_the_calls_own_gates():
    import test_gpu_composite_sweeps as CS
    op, plain_op = operator('3x3', ON), operator('3x3')
    try:
        unshadowed = arrays(plain_op.simulate_rays(AZ, EL))
        plain = arrays(op.simulate_rays(AZ, EL))
        spec = CS.spec_for(plain, AZ)
        res = op.simulate_rays_composite(AZ, EL, spec, keep_gates=True)
        got, gates = CS.maps_of(res), arrays(res)
        for k, v in plain.items():
            assert same_bits(gates[k], v), k
        CS.assert_maps(got, CS.rule(spec, [(gates, AZ)]), spec, 'shadowed composite')
        # ... and they are not the unshadowed operator's maps
        other = CS.maps_of(plain_op.simulate_rays_composite(AZ, EL, spec))
        assert not CS.same(other['count']['ZH'], got['count']['ZH'])
        assert np.isfinite(unshadowed['ZH']).sum() > np.isfinite(plain['ZH']).sum()
    finally:
        op.close()
        plain_op.close()


# ------------------------------------------------------------------ 5. the visibility
@pytest.mark.parametrize('name', ['one', '3x3', '7x7'])
def test_visibility(name):
    S = shadow_mod()
    A, B, V = operator(name), operator(name, ON), operator(name, {'terrain_visibility': 1})
    try:
        cols_a = A.interpolate_rays(AZ, EL, melting=False)
        n_sub = cols_a['mask'].shape[1]
        full, partial, untouched = preconditions(cols_a, n_sub)
        cols_b = B.interpolate_rays(AZ, EL, melting=False)
        w = cols_b['quad_weights']
        res = arrays(B.simulate_rays(AZ, EL))
        vis = res['visibility']
        assert vis.dtype == np.float64 and vis.shape == res['ZH'].shape
        assert same_bits(vis, S.visibility(cols_b['mask'], w))
        assert (vis[untouched] == 1.0).all()
        first = S.first_hit(cols_b['mask'])
        for r in full:
            assert (vis[r, first[r].max():] == 0.0).all() and not np.signbit(vis[r, first[r].max():]).any()
        if n_sub > 1:
            assert ((vis > 0) & (vis < 1))[partial].all()
        # without shadowing: the local below-topography sub-beams alone
        local = arrays(V.simulate_rays(AZ, EL))
        plain = arrays(A.simulate_rays(AZ, EL))
        assert V._ctx.launch_forms() == A._ctx.launch_forms()             # (the visibility alone changes no launch form)
        assert same_bits(local['visibility'], S.visibility(cols_a['mask'], w))
        assert (local['visibility'] >= vis).all() and (local['visibility'] > vis).any()
        for k in FIELDS:
            if k in local:
                assert same_bits(local[k], plain[k]), k
        # the column call makes it too, from the masks it is given
        got = arrays(B.simulate_columns(cols_b))
        assert same_bits(got['visibility'], vis)
        got = arrays(V.simulate_columns(strip(cols_a)))
        assert same_bits(got['visibility'], local['visibility'])
    finally:
        for op in (A, B, V):
            op.close()


def test_visibility_is_refused_under_scheme_ml():
    op = operator('ml', {'terrain_visibility': 1})
    try:
        with pytest.raises(ValueError):
            op.simulate_rays(AZ, EL)
        plain = operator('ml')
        cols = plain.interpolate_rays(AZ[:2], EL[:2], melting=False)
        plain.close()
        with pytest.raises(ValueError):
            op.simulate_columns(cols)
    finally:
        op.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_at_the_c_level_leave_the_context_usable():
    import ctypes
    import test_gpu_placement as P
    from cosmo_pol_amd import _native as N
    op = operator('3x3')
    try:
        ctx = op._ctx
        good, p, t, _ = P.spied(ctx, 'run_sweep', lambda: op.simulate_rays(AZ, EL))
        good = arrays(good)
        n = p.n_rays * p.n_gates
        zh, vis = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float64)

        def outputs(with_vis=False):
            o = N.Outputs()
            o.ZH = zh.ctypes.data
            if with_vis:
                o.visibility = vis.ctypes.data
            return o

        def refused(call, what):
            with pytest.raises(ValueError) as e:
                call()
            assert what in str(e.value), (what, str(e.value))
        for bad in (2, -1):
            q = N.SweepParams.from_buffer_copy(p)
            q.terrain_shadow, q.outputs_on_device = bad, 0
            refused(lambda: ctx.run_sweep(q, t, outputs()), 'terrain_shadow')
        # spaceborne geometry: a site table and the mode
        q = N.SweepParams.from_buffer_copy(p)
        q.terrain_shadow, q.outputs_on_device, q.geometry_mode = 1, 0, N.GEOM_SPACEBORNE
        site = np.zeros((p.n_rays, 8))
        t2 = N.RayTables.from_buffer_copy(t)
        t2.site, t2.version = site.ctypes.data, 0
        refused(lambda: ctx.run_sweep(q, t2, outputs()), 'spaceborne')
        # the column call: the caller's masks stand
        n_vars, n_sub = len(op._column_names()), 3
        col = np.zeros(n_sub * 4, dtype=np.float32)
        w3, sc = np.ones(n_sub), np.zeros(2 * n_sub)
        ptrs = (ctypes.c_void_p * n_vars)(*([col.ctypes.data] * n_vars))
        cc = N.Columns()
        cc.n_vars, cc.vals, cc.elev = n_vars, ctypes.cast(ptrs, ctypes.c_void_p), col.ctypes.data
        cc.sub_w, cc.az_sincos = w3.ctypes.data, sc.ctypes.data
        qc = N.SweepParams()
        qc.n_rays, qc.n_gates, qc.n_sub = 1, 4, n_sub
        qc.var_u, qc.var_v, qc.var_w, qc.var_rho = 0, 0, 0, -1
        zc, vc = np.zeros(4, dtype=np.float32), np.full(4, -7.0)
        oc = N.Outputs()
        oc.ZH, oc.visibility = zc.ctypes.data, vc.ctypes.data
        qc.terrain_shadow = 1
        refused(lambda: ctx.run_columns(qc, cc, oc), 'terrain_shadow')
        qc.terrain_shadow = 0                                # ... and without it the same call runs and makes the visibility
        ctx.run_columns(qc, cc, oc)
        ctx.synchronize()
        assert (vc == 1.0).all()
        # the visibility with per-gate weights
        ml = operator('ml')
        try:
            _, pm, tm, _ = P.spied(ml._ctx, 'run_sweep', lambda: ml.simulate_rays(AZ, EL))
            qm = N.SweepParams.from_buffer_copy(pm)
            qm.outputs_on_device = 0
            refused(lambda: ml._ctx.run_sweep(qm, tm, outputs(with_vis=True)), 'visibility')
            again = arrays(ml.simulate_rays(AZ, EL))
            assert np.isfinite(again['ZH']).any()
        finally:
            ml.close()
        # a plain sweep on the same context still works, and a shadowed one through the raw call too
        after = arrays(op.simulate_rays(AZ, EL))
        for k in FIELDS + GEOM:
            if k in good:
                assert same_bits(after[k], good[k]), k
        q = N.SweepParams.from_buffer_copy(p)
        q.terrain_shadow, q.outputs_on_device = 1, 0
        ctx.run_sweep(q, t, outputs(with_vis=True))
        ctx.synchronize()
        assert (vis == 0.0).any() and (vis == 1.0).any() and np.isnan(zh).sum() > np.isnan(good['ZH']).sum()
    finally:
        op.close()


def test_swaths_are_refused():
    op = operator('one', ON)
    try:
        with pytest.raises(NotImplementedError):
            op.get_GPM_swath({'Latitude': np.zeros((2, 2))})
    finally:
        op.close()


# ------------------------------------------------------------------ 7. the keys left off
@pytest.mark.parametrize('name', ['one', '3x3', 'melt_ice'])
def test_keys_absent_or_zero_change_nothing(name):
    A, Z = operator(name), operator(name, {'terrain_shadow': 0, 'terrain_visibility': 0})
    try:
        a, z = arrays(A.simulate_rays(AZ, EL)), arrays(Z.simulate_rays(AZ, EL))
        assert A._ctx.launch_forms() == Z._ctx.launch_forms()
        assert set(a) == set(z) and 'visibility' not in a
        for k, v in a.items():
            assert same_bits(z[k], v), (name, k)
        ca, cz = A.interpolate_rays(AZ, EL, melting=False), Z.interpolate_rays(AZ, EL, melting=False)
        assert set(ca) == set(cz)
        for k, v in ca.items():
            assert same_bits(cz[k], v), (name, 'export', k)
    finally:
        A.close()
        Z.close()


# ------------------------------------------------------------------ 8. the sharded volume path (two GPUs)
def test_sharded_volume_under_shadowing():
    """get_PPI of a distributed operator with both keys on, one rank per GPU over RCCL, against the same scan computed by every
    rank alone (tests/_shadow_dist_worker.py).  Needs two GPUs; skips itself otherwise."""
    import os
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('the sharded volume path under shadowing is run where two GPUs are visible')
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='1', CPOL_DIST_BACKEND='nccl', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29561', os.path.join(here, '_shadow_dist_worker.py')]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'SHADOW_DIST_OK world=2' in out.stdout
