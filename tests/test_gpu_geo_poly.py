"""The coordinate polynomials at every site, pole, range and grid edge (tests/_geopoly.py), on the device.

k_trajectory fits a degree-8 polynomial through 9 Chebyshev nodes per (ray, horizontal node); interp_gate evaluates two Horner
chains per gate and keeps the value when its guard says that c -+ 1..2 ulp fall into one cell inside the domain, and takes the long
form (Vincenty, atan2, asin) otherwise.  The other modules meet the polynomials at the benchmark's site, pole and range only.

  form A  sub-beam sweeps (3 x 3 nodes): every scenario twice, default and debug_flags = DEBUG_EXACT_SUBBEAMS (the long form for
          every sub-beam).  Over ALL sub-beam gates: masks, cell indices (tools/fast_sub_check.py::cell_index) and NaN patterns
          equal, coordinates at most 1 float32 ulp apart, sub_values bit-equal wherever both coordinates are; the coefficients
          (cpol_debug_read "geo_poly") are NaN exactly where host_fit rejects and follow the model to 1e-9 degrees over
          x in [-1, 1] elsewhere; every gate of a rejected fit has the long form's bits, every gate of an accepted one the bits of
          its polynomial (evaluated here from the device's coefficients) or, where the guard sent it on, the long form's; both
          runs within 1 ulp of exact_coords rounded, and in its cell except at the border gates counted by test_geo_poly_cpu.py.
  form B  single-beam sweeps (nh = nv = 1, device outputs, CPOL_GEO_POLY_CENTRAL=2 keeps the polynomials under the debug reads):
          the same; with host outputs the float64 lats / lons are the long form's bits.
  stale   150 km, 50 km, 150 km, another site, and the same rays under another range grid on one operator: a fresh operator's bits.
  shapes  the fit's launch at n_rays * n_h = 27 ... 57 fits, one ray, and 29 x 1 nodes, where its stride loop runs twice.

Every scenario writes one record to geo_poly_records.jsonl (gates, gates on polynomials, gates the guard sent to the long form,
rejected fits, worst ulp between the forms and against exact_coords).

On the commit before the tail rule (its library unchanged, these tests alone; "geo_poly" is unknown there, which _check reports
while the rest runs) the eight near-pole cases failed as the model predicts, in the coordinates and never in a cell or a mask:
  near_pole_50km_02   form A  12 865 of 59 400 coordinates beyond 1 ulp of the long form, 19 ulp at most; form B 1 741 of 6 600, 18 ulp
  near_pole_50km_075  form A  593 coordinates beyond 1 ulp, 3 ulp at most; form B 120, 3 ulp
  far_pole_500km      form A  6 180 coordinates beyond 1 ulp, 53 ulp at most; form B 917, 52 ulp
  near_pole_3deg      1 ulp at most in both forms: only "a fit that host_fit rejects differs from the long form" (141 / 24 gates by 1 ulp:
                      fits the tail rule now rejects) and the missing hook
each with the same figures against exact_coords ("default: 19 ulp from exact_coords"), the long form within 1 ulp of it throughout.

Tried against scratch builds with one edit each (cpol_interp.inl, cosmo_pol_hip.hip); each leaves wrong numbers, none an index out
of bounds -- a coordinate, however wrong, passes the gate kernel's own domain test before it becomes an index:
  * both sanity rules removed (`sane` stays true): rlon_wrap fails in both forms -- 33 / 11 verdicts, masks of 61 / 11 gates, cells of
    240 / 30 gates, coordinates 48 061 ulp apart;
  * `spans` without its two domain terms: rlon_wrap fails in both forms (16 / 1 gates of accepted fits extrapolated over +-180: the
    polynomial says 180.0003, the long form -179.9997; masks agree, both are outside).  leaves_domain PASSES: a polynomial value
    beyond the border fails the gate kernel's domain test like the long form's -- the two terms matter where the forms round to
    different sides of a border, which no gate of it does;
  * the fit's stride loop cut to one trip (`break` after the second barrier): the two 29 x 1 shapes fail at the coefficients alone
    ("coefficients 1.5e+17 degrees from the model": the array's unwritten rows) -- the guard sends all 200 gates of such a fit to the
    long form, so that coordinates, cells and masks stay right; the seven other shapes pass;
  * `set->poly_scale != geo_poly_scale` left out of the rebuild key: the stale-state test fails at its first range-grid step
    ("range0 60750", coordinates); its four steps through the configuration pass, each being a new table version."""
import copy

import numpy as np
import pytest

import _geopoly as G
from test_gpu_rough_tables import _record

pytestmark = pytest.mark.gpu

KNOBS = ('CPOL_GEO_POLY', 'CPOL_GEO_POLY_CENTRAL', 'CPOL_USE_GRAPH', 'CPOL_INTERP_XCD_RAYS')


def _operator(monkeypatch, scn, single):
    from cosmo_pol_amd import RadarOperator
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if single:
        monkeypatch.setenv('CPOL_GEO_POLY_CENTRAL', '2')
    op = RadarOperator(config=scn.conf, luts=scn.luts(), output_variables='only_radar', lanes=1)
    c = scn.cube
    op.load_model_arrays(c['data'], c['zlevels'], c['proj_info'], c['resolution'])
    return op


def _slab(scn):
    import torch
    from cosmo_pol_amd.radar_operator import RADAR_FIELDS
    slab = torch.full((len(RADAR_FIELDS), len(scn.az), scn.n_gates), float('nan'), dtype=torch.float32, device='cuda')
    return slab, {k: slab[i].data_ptr() for i, k in enumerate(RADAR_FIELDS)}


def _sweep(op, scn, exact, single, call=None):
    """One sweep under the debug reads -> dict(coords [n_rays, n_sub, n_gates, 2], mask, vals [n_vars, ...], s32 [n_rays, n_v, n_gates],
    poly [n_rays, n_h, 2, 9] or None (the long form, or a library without the hook), out: the radar fields)."""
    from cosmo_pol_amd import _native as N
    sub = scn.sub()
    n_rays, n_sub, ng = len(scn.az), sub.n_sub, scn.n_gates
    op.debug_flags = N.DEBUG_EXACT_SUBBEAMS if exact else 0
    op._ctx.enable_debug(True)
    raised, out = False, None
    try:
        if call is not None:
            out = call()
        elif single:
            slab, ptrs = _slab(scn)
            op.simulate_rays(scn.az, scn.el, device_outputs=ptrs)
            op.wait()
            out = slab.cpu().numpy()
        else:
            res = op.simulate_rays(scn.az, scn.el)
            out = np.stack([res[k] for k in ('ZH', 'ZDR', 'KDP', 'RVEL')]).astype(np.float64)
    except IndexError:
        raised = True
    assert raised == scn.leaves, 'IndexError %s, gates outside the cube %s' % (raised, scn.leaves)
    forms = op._ctx.launch_forms()
    assert forms['n_sub'] == n_sub
    n_vars = len(op._staged_vars)
    d = {'coords': op._ctx.debug_read('sub_coords', (n_rays, n_sub, ng, 2), np.float32),
         'mask': op._ctx.debug_read('sub_mask', (n_rays, n_sub, ng), np.int8),
         'vals': op._ctx.debug_read('sub_values', (n_vars, n_rays, n_sub, ng), np.float32),
         's32': op._ctx.debug_read('traj', (n_rays, len(sub.pts_ver), 3, ng), np.float32)[:, :, 0].copy(),
         'forms': forms, 'out': out, 'poly': None, 'hook': True}
    if not exact:
        try:
            d['poly'] = op._ctx.debug_read('geo_poly', (n_rays, len(sub.pts_hor), 2, G.NP), np.float64)
        except (ValueError, N.NativeError) as e:              # (a library from before the hook: _check reports it, the rest runs)
            assert 'unknown buffer' in str(e), e
            d['hook'] = False
    op._ctx.enable_debug(False)
    op.debug_flags = 0
    return d


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _poly32(scn, poly, s32, sub):
    """float32 of the device's Horner chains from ITS coefficients (extended precision here: the float32 cast hides the rest)."""
    r = scn.conf['radar']
    scale = 2.0 / ((r['radial_resolution'] / 2. + (scn.n_gates - 1) * float(r['radial_resolution'])) * 1.001)
    x = (s32.astype(np.float64)[:, sub.sub_v] * scale - 1.0).astype(np.longdouble)          # [n_rays, n_sub, n_gates]
    c = poly[:, sub.sub_h].astype(np.longdouble)                                               # [n_rays, n_sub, 2, 9]
    acc = np.zeros(c.shape[:3] + (x.shape[-1],), np.longdouble)
    with np.errstate(invalid='ignore'):
        for q in range(G.NP - 1, -1, -1):
            acc = acc * x[:, :, None, :] + c[..., q][..., None]
    return np.moveaxis(acc, 2, -1).astype(np.float64).astype(np.float32)


def _guard(scn, p32):
    """interp_gate's `spans` over float32 polynomial values, for the records: True where the guard sends the gate to the long form
    (c -+ 2^-23 max(|c|, |llc|) in two cells, or outside the domain; the quotient as a float32 division)."""
    out = np.zeros(p32.shape[:-1], bool)
    pr = scn.proj
    with np.errstate(invalid='ignore', over='ignore'):
        for j, (llc, urc, res) in enumerate(((pr['La1'], pr['La2'], scn.res[1]), (pr['Lo1'], pr['Lo2'], scn.res[0]))):
            c, llc, urc, res = p32[..., j], np.float32(llc), np.float32(urc), np.float32(res)
            d = np.maximum(np.maximum(np.abs(c), np.abs(llc)), np.float32(1e-30)) * np.float32(1.1920929e-7)
            lo, hi = c - d, c + d
            out |= (np.floor((lo - llc) / res) != np.floor((hi - llc) / res)) | ~(lo >= llc) | ~(hi <= urc)
    return out


def _check(scn, dflt, long_, tag):
    """Every assertion of forms A and B; failures are collected so that one run names all of them.  -> the scenario's record."""
    sub = scn.sub()
    fit = scn.fit()
    fails = []

    def want(ok, what):
        if not ok:
            fails.append(what)

    cd, cl = dflt['coords'], long_['coords']
    n_gates = int(dflt['mask'].size)
    want(np.array_equal(dflt['s32'], long_['s32']), 'ray paths differ between the runs')
    want(np.array_equal(dflt['mask'], long_['mask']), 'masks differ in %d gates' % int((dflt['mask'] != long_['mask']).sum()))
    want(np.array_equal(np.isnan(cd), np.isnan(cl)), 'NaN patterns of the coordinates differ')
    want(np.array_equal(np.isnan(dflt['vals']), np.isnan(long_['vals'])), 'NaN patterns of the values differ')
    fin = np.isfinite(cd).all(axis=-1) & np.isfinite(cl).all(axis=-1)
    i_d, i_l = G.cell_index(cd, scn.proj, scn.res), G.cell_index(cl, scn.proj, scn.res)
    cells = ((i_d[0] != i_l[0]) | (i_d[1] != i_l[1])) & fin
    want(not cells.any(), 'cell indices differ in %d gates' % int(cells.sum()))
    ulp = G.ulp_distance(cd[fin], cl[fin])
    worst = int(ulp.max()) if ulp.size else 0
    want(worst <= 1, 'coordinates %d ulp apart (%d coordinates beyond 1 ulp)' % (worst, int((ulp > 1).sum())))
    same = (_bits(cd) == _bits(cl)).all(axis=-1)
    vals_ok = (_bits(dflt['vals']) == _bits(long_['vals']))[:, same]
    want(vals_ok.all(), 'sub_values differ at %d gates whose coordinates have the same bits' % int((~vals_ok).any(axis=0).sum()))
    # ---- the fits: verdicts and coefficients against the model
    sane = fit['sane']
    poly = dflt['poly']
    on_poly = by_guard = guard_moved = -1
    want(dflt['hook'], 'cpol_debug_read "geo_poly" is unknown to this library: verdicts and coefficients unchecked')
    if poly is not None:
        dev_sane = np.isfinite(poly).all(axis=(-1, -2))
        want(np.array_equal(np.isnan(poly).any(axis=(-1, -2)), ~dev_sane), 'a fit is partly NaN')
        want(np.array_equal(dev_sane, sane), 'verdicts differ from host_fit in %d of %d fits (device accepts %d, the model %d)'
             % (int((dev_sane != sane).sum()), sane.size, int(dev_sane.sum()), int(sane.sum())))
        both = dev_sane & sane
        x = np.linspace(-1.0, 1.0, 33)
        dv = np.zeros(poly.shape[:3] + (len(x),))
        for q in range(G.NP - 1, -1, -1):
            dv = dv * x + (np.nan_to_num(poly[..., q]) - fit['coef'][..., q])[..., None]
        dev = float(np.abs(dv[both]).max()) if both.any() else 0.0
        want(dev <= 1e-9, 'coefficients %.3g degrees from the model' % dev)
        # ---- which form every gate took
        p32 = _poly32(scn, poly, dflt['s32'], sub)
        acc = dev_sane[:, sub.sub_h][:, :, None] & np.ones(cd.shape[:-1], bool)
        is_poly = (_bits(cd) == _bits(p32)).all(axis=-1)
        want((same | acc).all(), 'a gate of a rejected fit differs from the long form')
        want((is_poly | same)[acc].all(), '%d gates of accepted fits have neither their polynomial\'s bits nor the long form\'s'
             % int((~(is_poly | same))[acc].sum()))
        # (a gate the guard sends on mostly gets the same bits from the long form: the guard itself is emulated for the record)
        sent = _guard(scn, p32) & acc
        on_poly, by_guard, guard_moved = int((acc & ~sent).sum()), int(sent.sum()), int((~is_poly & acc).sum())
        want(not sane.any() or on_poly > 0, 'no gate took a polynomial')
    rej = ~sane[:, sub.sub_h]
    want(same[rej].all(), '%d gates of fits that host_fit rejects differ from the long form' % int((~same[rej]).sum()))
    # ---- both runs against the float64 reference
    ex = G.exact_coords(scn.site, scn.pole, G.node_azimuths(scn.conf, scn.az), dflt['s32'], sub.sub_h, sub.sub_v)
    ex32 = ex.astype(np.float32)
    border = G.border_gates(ex, scn.proj, scn.res)
    i_x = G.cell_index(ex32, scn.proj, scn.res)
    worst_x = 0
    for name, c, idx in (('default', cd, i_d), ('long form', cl, i_l)):
        f = np.isfinite(c).all(axis=-1)
        want(f.all(), '%s: %d gates without coordinates' % (name, int((~f).sum())))
        u = G.ulp_distance(c[f], ex32[f])
        worst_x = max(worst_x, int(u.max()))
        want(u.max() <= 1, '%s: %d ulp from exact_coords (%d coordinates beyond 1 ulp)' % (name, int(u.max()), int((u > 1).sum())))
        off = ((idx[0] != i_x[0]) | (idx[1] != i_x[1])) & f & ~border
        want(not off.any(), '%s: %d gates away from every border in another cell than exact_coords' % (name, int(off.sum())))
    inside = G.in_domain(ex32.astype(np.float64), scn.proj)
    disagree = ((long_['mask'] == 2) == inside) & ~border
    want(not disagree.any(), 'mask 2 and the domain test of exact_coords disagree at %d gates away from the border' % int(disagree.sum()))
    rec = {'scenario': scn.name, 'form': tag, 'gates': n_gates, 'gates_on_polynomials': on_poly, 'gates_sent_on_by_the_guard': by_guard,
           'of_those_with_other_bits_than_the_polynomial': guard_moved,
           'fits': int(sane.size), 'rejected_fits_model': int((~sane).sum()),
           'rejected_fits_device': int((~np.isfinite(poly).all(axis=(-1, -2))).sum()) if poly is not None else -1,
           'node_rule_alone_would_accept': int(fit['sane_nodes'].sum()), 'worst_ulp_between_forms': worst,
           'coordinates_beyond_1_ulp': int((ulp > 1).sum()), 'cells_that_differ': int(cells.sum()),
           'masks_that_differ': int((dflt['mask'] != long_['mask']).sum()), 'worst_ulp_against_exact': worst_x,
           'border_gates': int(border.sum()), 'failed': fails}
    _record(rec, 'geo_poly_records.jsonl', 'GEO_POLY')
    assert not fails, (scn.name, tag, fails)
    return rec


@pytest.mark.parametrize('name', G.NAMES)
def test_form_a_subbeam_sweeps_follow_the_long_form(monkeypatch, name):
    scn = G.scenario(name)
    op = _operator(monkeypatch, scn, single=False)
    dflt = _sweep(op, scn, exact=False, single=False)
    long_ = _sweep(op, scn, exact=True, single=False)
    op.close()
    assert dflt['forms']['n_sub'] == 9 and dflt['forms']['poly_central'] == 0
    _check(scn, dflt, long_, 'A')


@pytest.mark.parametrize('name', G.NAMES)
def test_form_b_single_beam_sweeps_follow_the_long_form(monkeypatch, name):
    scn = G.scenario(name).with_quadrature(1, 1)
    op = _operator(monkeypatch, scn, single=True)
    dflt = _sweep(op, scn, exact=False, single=True)
    assert dflt['forms']['poly_central'] == 1 and dflt['forms']['n_sub'] == 1
    long_ = _sweep(op, scn, exact=True, single=True)
    assert long_['forms']['poly_central'] == 0
    _check(scn, dflt, long_, 'B')
    if not scn.leaves:
        # host outputs: the grid coordinates still come from the polynomials, the float64 latitude / longitude are the long form's bits
        res = op.simulate_rays(scn.az, scn.el)
        assert op._ctx.launch_forms()['poly_central'] == 1
        from cosmo_pol_amd import _native as N
        op.debug_flags = N.DEBUG_EXACT_SUBBEAMS
        for k in [k for k in op._cache if isinstance(k, tuple) and k[0] == 'geom']:
            del op._cache[k]
        ref = op.simulate_rays(scn.az, scn.el)
        assert op._ctx.launch_forms()['poly_central'] == 0
        op.debug_flags = 0
        assert np.isfinite(ref['lats']).all()
        for k in ('lats', 'lons', 'dist', 'heights'):
            assert np.array_equal(res[k], ref[k], equal_nan=True), k
    op.close()


def _outputs(op, scn, call=None):
    d = _sweep(op, scn, exact=False, single=True, call=call)
    return d


def _same_bits(a, b, what):
    for k in ('coords', 'mask', 'vals', 'out'):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    if a['poly'] is not None and b['poly'] is not None:
        assert np.array_equal(a['poly'], b['poly'], equal_nan=True), (what, 'poly')


def test_one_operator_through_ranges_sites_and_range_grids_gives_a_fresh_operators_bits(monkeypatch):
    """The polynomials of a single-beam sweep belong to the resident table set of its rays; they are made again when its range grid
    (poly_scale) or its site (poly_site) changes.  150 km, 50 km, 150 km and another site through the configuration (each a new
    set of ray tables on the host: the library meets another version as well), then -- the one way to a new poly_scale under an
    unchanged version and shape -- the same rays over another first range, as a caller of cpol_run_sweep may.  Each step gives the
    bits of a fresh operator, and the long form's cells."""
    from cosmo_pol_amd import _native as N
    base = G.scenario('long_range').with_quadrature(1, 1)          # (a cube that holds 150 km)
    lat, lon = G.geodesy.rotated_to_wgs(0.9, -2.6, G.POLE[0], G.POLE[1])

    def variant(rng, step, site=None):
        conf = copy.deepcopy(base.conf)
        conf['radar'].update(range=rng, radial_resolution=step)
        if site is not None:
            conf['radar']['coords'] = list(site)
        return G.Scenario('stale_%d' % rng, conf, base.cube, base.az, base.el, leaves=False)

    steps = [variant(150000, 1500), variant(50000, 500), variant(150000, 1500), variant(150000, 1500, (float(lat), float(lon), 700.0))]
    op = _operator(monkeypatch, steps[0], single=True)
    for k, scn in enumerate(steps):
        if k:
            op.config = scn.conf
        got = _outputs(op, scn)
        assert got['forms']['poly_central'] == 1
        fresh_op = _operator(monkeypatch, scn, single=True)
        fresh = _outputs(fresh_op, scn)
        long_ = _sweep(fresh_op, scn, exact=True, single=True)
        fresh_op.close()
        _same_bits(got, fresh, 'step %d' % k)
        assert np.array_equal(got['mask'], long_['mask'])
        assert G.ulp_distance(got['coords'], long_['coords']).max() <= 1
    # ---- the same rays, version and shape over another range grid: only poly_scale tells the library
    scn = steps[-1]
    step = float(scn.conf['radar']['radial_resolution'])
    coords = scn.conf['radar']['coords']

    def shifted(o, range0):
        def call():
            slab, ptrs = _slab(scn)
            o._run_rays(scn.az, scn.el, coords, scn.n_gates, range0, N.GEOM_GROUND_43, device_outputs=ptrs)
            o.wait()
            return slab.cpu().numpy()
        return call
    for range0 in (step / 2. + 40 * step, step / 2.):
        got = _outputs(op, scn, call=shifted(op, range0))
        fresh_op = _operator(monkeypatch, scn, single=True)
        fresh = _outputs(fresh_op, scn, call=shifted(fresh_op, range0))
        fresh_op.close()
        assert got['forms']['poly_central'] == 1
        _same_bits(got, fresh, 'range0 %g' % range0)
    op.close()


@pytest.mark.parametrize('nh, nv, n_rays', G.SHAPES)
def test_launch_shapes_of_the_fit(monkeypatch, nh, nv, n_rays):
    """28 fits per workgroup, n_rays * n_v workgroups: fits one below, at and one above a workgroup's and two workgroups' share, one
    ray, and 29 x 1 nodes -- the only shape with more fits than the grid holds, whose fits 28 and above are made in the stride
    loop's second trip (between its two barriers) and must be finite, the model's, and in use."""
    scn = G.scenario('control').with_quadrature(nh, nv, n_rays)
    op = _operator(monkeypatch, scn, single=False)
    dflt = _sweep(op, scn, exact=False, single=False)
    long_ = _sweep(op, scn, exact=True, single=False)
    op.close()
    rec = _check(scn, dflt, long_, 'shape %dx%d' % (nh, nv))
    assert rec['rejected_fits_model'] == 0
    if nh == 29:
        sub = scn.sub()
        poly = dflt['poly']
        flat = poly.reshape(-1, 2, G.NP)
        second_trip = np.arange(len(flat)) >= 28 * n_rays * nv       # (fit e is made by workgroup (e / 28) % grid in trip e / (28 grid))
        assert second_trip.sum() == n_rays and np.isfinite(flat[second_trip]).all()
        p32 = _poly32(scn, poly, dflt['s32'], sub)
        is_poly = (_bits(dflt['coords']) == _bits(p32)).all(axis=-1)                       # [n_rays, n_sub, n_gates]
        fit_of = (np.arange(n_rays)[:, None] * nh + sub.sub_h[None, :])                     # [n_rays, n_sub]
        central = sub.central
        for e in np.nonzero(second_trip)[0]:
            sel = (fit_of == e) & (np.arange(sub.n_sub) != central)[None, :]
            if sel.any():
                assert is_poly[sel].sum() >= 0.9 * is_poly[sel].size, (e, int(is_poly[sel].sum()))
        # (one ray: its one fit of the second trip belongs to the outermost node, whose weight of 1e-20 falls to the weight threshold --
        # the coefficient check above is all that sees it; three rays: nodes 26 and 27 of the last ray carry sub-beams)
        used = [e for e in np.nonzero(second_trip)[0] if ((fit_of == e) & (np.arange(sub.n_sub) != central)[None, :]).any()]
        assert n_rays == 1 or len(used) >= 2
