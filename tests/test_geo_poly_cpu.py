"""The host model of the coordinate polynomials and its scenarios (tests/_geopoly.py) on their own, without a GPU: what
tests/test_gpu_geo_poly.py relies on when it holds the device against them, so that no GPU test can pass by leaving cases out.

Counts of the model (float64 NumPy; errors in float32 ulp of the coordinate).  The planted rays are chosen among 1440 azimuths by
their central node's fit; the fits counted are those of all three horizontal nodes of the chosen rays:

  scenario             rays  planted > 2 ulp off  worst     fits  node rule accepts  tail rule accepts  worst behind both rules
  near_pole_50km_02    33    20                   18 ulp    99    59                 1                  9e-7 ulp
  near_pole_50km_075   34    6                    2.4 ulp   102   61                 21                 0.0025 ulp
  near_pole_3deg       28    0 (worst 0.07 ulp)   --        84    46                 22                 0.0041 ulp
  far_pole_500km       38    10                   52 ulp    114   72                 12                 0.0024 ulp

Over 720 azimuths the node rule alone leaves 315 ulp at 0.1 degrees from the pole (50 km) and 1037 ulp at 0.2 degrees (150 km).
Border gates (exact coordinate within 2 ulp of a cell or domain border, inside the domain): at most 0.3 % of a scenario's
sub-beam gates (southern 126, rlon_wrap 110 of 43 200); fine_grid has 69."""
import numpy as np
import pytest

import _geopoly as G

SOUND = [n for n in G.NAMES if n not in G.NEAR_POLE]


def _poly_error(scn):
    """(error [n_rays, n_sub, n_gates, 2] of the fits against exact_coords in float32 ulp of the exact coordinate, exact, fit, sub)."""
    f, sub = scn.fit(), scn.sub()
    s32 = scn.host_traj()
    ex = scn.exact(s32)
    x = 2.0 * s32.astype(np.float64)[:, sub.sub_v] / scn.s_max - 1.0
    c = f['coef'][:, sub.sub_h]
    acc = np.zeros(c.shape[:3] + (x.shape[-1],))
    for q in range(G.NP - 1, -1, -1):
        acc = acc * x[:, :, None, :] + c[..., q][..., None]
    return np.abs(np.moveaxis(acc, 2, -1) - ex) / G.ulp32(ex), ex, f, sub


def test_fit_matrix_reproduces_polynomials_of_degree_8():
    rng = np.random.default_rng(5)
    c = rng.normal(size=(7, G.NP))
    vals = np.stack([np.polyval(ci[::-1], G.NODES) for ci in c])
    assert np.allclose(np.einsum('pq,nq->np', G.FIT_M, vals), c, rtol=0, atol=1e-12)
    # the Chebyshev coefficients of the rule from the two highest monomial ones
    from numpy.polynomial import chebyshev
    for ci in c:
        ch = chebyshev.poly2cheb(ci)
        assert abs(ch[8] - ci[8] / 128.0) < 1e-14 and abs(ch[7] - ci[7] / 64.0) < 1e-14


def test_exact_coords_take_the_sub_beams_nodes():
    scn = G.scenario('control')
    sub = scn.sub()
    assert sub.n_sub == 9 and len(sub.pts_hor) == 3
    s32 = scn.host_traj()
    ex = scn.exact(s32)
    assert ex.shape == (48, 9, 100, 2)
    k = 5
    one = G.exact_at(scn.site, scn.pole, scn.az[7] + sub.pts_hor[sub.sub_h[k]], s32[7, sub.sub_v[k]].astype(np.float64))
    assert np.array_equal(ex[7, k], one)
    # ... and the rotation is the oracle's before its float32 cast
    from cosmo_pol_oracle import geodesy
    lat, lon = geodesy.wgs84_direct(scn.site[0], scn.site[1], scn.az[7], 12345.0)
    r32 = geodesy.wgs_to_rotated(np.array([lat]), np.array([lon]), *scn.pole)[0]
    r64 = G.exact_at(scn.site, scn.pole, scn.az[7], 12345.0)
    assert np.array_equal(r64.astype(np.float32), r32)


@pytest.mark.parametrize('name', SOUND)
def test_sound_scenarios_accept_every_fit_within_a_hundredth_of_an_ulp(name):
    """Every fit of the scenarios away from the rotated pole passes BOTH rules and follows exact_coords to 0.01 float32 ulp at every
    gate.  rlon_wrap is the one exception by design: the fits whose nodes straddle +-180 are rejected by the node rule (at least
    6 are, at least 60 are not), and an accepted fit is compared with the exact longitude unwrapped onto the fit's side."""
    scn = G.scenario(name)
    err, ex, f, sub = _poly_error(scn)
    assert np.array_equal(f['sane'], f['sane_nodes'])          # the tail rule rejects nothing here
    if name == 'rlon_wrap':
        assert (~f['sane']).sum() >= 6 and f['sane'].sum() >= 60
        jump = np.abs(np.diff(f['nodes'][~f['sane']][:, 1], axis=-1)).max(axis=-1)
        assert (jump > 359.0).all()
        ok = f['sane'][:, sub.sub_h]
        unwrapped = ex.copy()
        unwrapped[..., 1] = np.where(ex[..., 1] < 0, ex[..., 1] + 360.0, ex[..., 1])
        wrapped_gate = ok[:, :, None] & (ex[..., 1] < 0)
        assert wrapped_gate.sum() >= 3                          # accepted fits extrapolated over the wrap
        err[..., 1] = np.where(ex[..., 1] < 0, 0.0, err[..., 1])
        assert err[ok].max() < 0.01, err[ok].max()
        return
    assert f['sane'].all()
    assert err.max() < 0.01, err.max()


@pytest.mark.parametrize('name', G.NEAR_POLE)
def test_near_pole_scenarios_plant_wrong_rays_behind_the_node_rule(name):
    """Rays that the node rule (the only rule before the tail rule) accepts and that are more than 2 ulp off: at least 6 where the
    model finds that many among 1440 azimuths (50 km at 0.2 and 0.75 degrees, 500 km at 6 degrees), none at 3 degrees and
    150 km -- there accepted and rejected rays are mixed and every accepted one is sound.  The tail rule rejects every planted ray
    and every fit it accepts follows exact_coords to 0.01 ulp."""
    scn = G.scenario(name)
    err, ex, f, sub = _poly_error(scn)
    per_fit = np.zeros(f['sane'].shape)
    for k in range(sub.n_sub):
        per_fit[:, sub.sub_h[k]] = np.maximum(per_fit[:, sub.sub_h[k]], err[:, k].max(axis=(-1, -2)))
    central = len(sub.pts_hor) // 2
    bad = scn.planted['bad']
    assert f['sane_nodes'][bad, central].all() and (len(bad) == 0 or per_fit[bad, central].min() > 2.0)
    if name == 'near_pole_3deg':
        assert len(bad) == 0
        assert per_fit[f['sane_nodes']].max() < 1.0
        assert f['sane_nodes'].sum() >= 20 and (~f['sane_nodes']).sum() >= 20
    else:
        assert len(bad) >= 6, len(bad)
        # ... with gates inside the domain, so that a wrong coordinate can show as a wrong cell
        inside = G.in_domain(ex, scn.proj)[bad][:, sub.sub_h == central]
        assert inside.sum() >= 100 * len(bad) // 2
    assert (~f['sane_nodes'][scn.planted['rejected'], central]).all() and len(scn.planted['rejected']) >= 6
    assert f['sane_nodes'][scn.planted['sound'], central].all() and len(scn.planted['sound']) >= 1
    assert not f['sane'][bad].any()
    assert f['sane'].sum() >= 1                                 # (the polynomials stay in use)
    assert per_fit[f['sane']].max() < 0.01, per_fit[f['sane']].max()
    print('GEO_POLY_CPU', name, dict(rays=len(scn.az), planted_bad=len(bad), worst_planted_ulp=float(per_fit[bad, central].max()) if len(bad) else 0.0,
                                    node_rule_accepts=int(f['sane_nodes'].sum()), tail_rule_accepts=int(f['sane'].sum()), fits=int(f['sane'].size),
                                    worst_ulp_behind_the_tail_rule=float(per_fit[f['sane']].max())))


@pytest.mark.parametrize('dist_deg, rng, wrong', [(0.1, 50000, True), (0.2, 50000, True), (0.75, 50000, True), (1.0, 150000, False),
                                                   (2.0, 150000, True), (0.2, 150000, True), (3.0, 500000, True), (6.0, 500000, True),
                                                   (10.0, 500000, False)])
def test_tail_rule_leaves_no_wrong_ray_among_720_azimuths(dist_deg, rng, wrong):
    """Sites at dist_deg from the rotated pole, 720 azimuths each: whatever passes both rules is within 0.01 ulp of the exact
    function at 400 points of the ray; where `wrong`, the node rule alone lets rays through that are more than 2 ulp off."""
    from cosmo_pol_oracle import geodesy
    np_lat, np_lon = geodesy.wgs84_direct(G.SITE[0], G.SITE[1], 90.0, dist_deg * G.DEG * 6371000.0)
    pole = (-float(np_lat), float(np_lon) - 180.0)
    s_max = 1.001 * (rng - rng / 200.0)
    az = np.arange(720) * 0.5
    f = G.host_fit(G.SITE, pole, az[:, None], s_max)
    s = np.linspace(0.0, s_max / 1.001, 400)[None, :].repeat(len(az), 0)
    ex = G.exact_at(G.SITE, pole, az[:, None], s)
    err = (np.abs(G.poly_at(f['coef'], s, s_max)[:, 0] - ex) / G.ulp32(ex)).max(axis=(1, 2))
    old, new = f['sane_nodes'][:, 0], f['sane'][:, 0]
    print('GEO_POLY_CPU', dist_deg, rng, dict(node_rule_accepts=int(old.sum()), more_than_2_ulp_off=int((old & (err > 2)).sum()),
                                             worst_ulp=float(err[old].max()), tail_rule_accepts=int(new.sum()),
                                             worst_ulp_behind_the_tail_rule=float(err[new].max()) if new.any() else 0.0))
    assert not wrong or (old & (err > 2.0)).sum() >= 1
    assert not new.any() or err[new].max() < 0.01


@pytest.mark.parametrize('name', G.NAMES)
def test_no_fit_sits_at_a_rules_threshold(name):
    """Device and model then agree on every verdict although their sincos may differ in the last bit: no node difference within
    1e-6 degrees of the node rule's 1.0, no tail within 1 % of the tail rule's threshold (the tail is a difference of node values
    of a few degrees times 1e-16: its rounding noise is ~1e-6 of the threshold)."""
    scn = G.scenario(name)
    for shape in [(3, 3), (1, 1)]:
        f = scn.with_quadrature(*shape).fit()
        assert np.abs(f['node_step'] - G.RULE_NODE_STEP).min() > 1e-6
        r = G.tail_ratio(f)[f['sane_nodes']]
        assert np.abs(r - 1.0).min() > 1e-2, np.abs(r - 1.0).min()


@pytest.mark.parametrize('name', G.NAMES)
def test_border_gates_are_few(name):
    """Gates whose exact coordinate lies within 2 ulp of a cell border or of the domain border -- where two correct roundings may
    sit in different cells, and which the GPU test therefore exempts from its comparison of cell indices with exact_coords -- are
    at most 2 % of a scenario; fine_grid, made for them, has at least 20."""
    scn = G.scenario(name)
    ex = scn.exact()
    b = G.border_gates(ex, scn.proj, scn.res) & G.in_domain(ex, scn.proj)
    print('GEO_POLY_CPU', name, dict(gates=int(b.size), border_gates=int(b.sum()), share=float(b.mean())))
    assert b.mean() <= 0.02
    if name == 'fine_grid':
        assert b.sum() >= 20
    inside = G.in_domain(ex, scn.proj)
    assert scn.leaves == (not inside.all()) and inside.mean() > 0.3
    assert scn.leaves or name not in ('leaves_domain', 'rlon_wrap')


def test_leaves_domain_leaves_on_all_four_sides():
    scn = G.scenario('leaves_domain')
    ex = scn.exact()
    p = scn.proj
    assert (ex[..., 0] < p['La1']).any() and (ex[..., 0] > p['La2']).any() and (ex[..., 1] < p['Lo1']).any() and (ex[..., 1] > p['Lo2']).any()


def test_launch_shapes_cover_the_fits_per_workgroup():
    counts = sorted(n * nh for nh, nv, n in G.SHAPES)
    for want in (27, 28, 29, 56, 57):
        assert want in counts
    assert (3, 3, 1) in G.SHAPES
    # 28 fits per workgroup, n_rays * n_v workgroups: only (29, 1) strides
    assert [(nh, nv) for nh, nv, n in G.SHAPES if n * nh > 28 * n * nv] == [(29, 1), (29, 1)]
    scn = G.scenario('control').with_quadrature(29, 1, 3)
    # (the two outermost of 29 nodes weigh 1e-20 and fall to the weight threshold's rounding: fitted all the same)
    assert len(scn.sub().pts_hor) == 29 and scn.sub().n_sub >= 27 and len(scn.az) == 3
