"""Network composites on the GPU through the sweeps: a composite on the geographic plane, the model's rotated plane and a
callable plane against composite.compose / composite.finish of the call's own per-gate arrays and composite.plane_xy of its own
`lats` / `lons`, exactly (NaNs positionally equal); the rest of such a call against the same call without a composite; the plane
store across repeat calls; two radars folded into one pass with their sources; the scores of a network pass; the ensemble.

Cases: the golden radials c2_rsg (single beam) and c4_7x7 (49 sub-beams) on cube 0, seven rays at az + 0.5 k.  The grid spans the
gates of a first plain call on the plane at hand, built as test_gpu_composite_sweeps.spec_for builds it (a few cells beyond the
gates stay empty), so that no test passes on an empty map."""
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_ensemble import case, load, operator
from test_gpu_composite_sweeps import assert_maps, finite_quantiles, maps_of, plain_run, same, same_gates
from test_gpu_histogram_sweeps import arrays, op_for, rays, _ops

pytestmark = pytest.mark.gpu

NAMES = ['c2_rsg', 'c4_7x7']
FIELDS = ['ZH', 'KDP', 'ATT_V']


def CP():
    from cosmo_pol_amd import composite
    return composite


def NB():
    from cosmo_pol_amd import neighbourhood
    return neighbourhood


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def pole_of(name):
    p = case(name)[2][0]['proj_info']
    return (float(p['Latitude_of_southern_pole']), float(p['Longitude_of_southern_pole']))


def local_metres(lats, lons):
    """A projection of the user's: metres east and north of (46.5 N, 7.5 E) on a plane tangent there (float32 on purpose on
    one axis: the plane is taken as it comes)."""
    return (lons - 7.5) * (111.2e3 * np.cos(np.deg2rad(46.5))), ((lats - 46.5) * 111.2e3).astype(np.float32)


def xy_of(plane, gates, name):
    return CP().plane_xy(plane, gates['lats'], gates['lons'], pole_of(name) if plane == 'model' else None)


def spec_on(plane, name, gate_sets, products=('max', 'lowest', 'echo_top'), slab=True, fields=FIELDS, n=(9, 7)):
    """A grid on `plane` over the gates of `gate_sets` (non-uniform, one ring of cells beyond them), thresholds and slab from the
    data: test_gpu_composite_sweeps.spec_for with the plane's own coordinates."""
    xs, ys = zip(*(xy_of(plane, g, name) for g in gate_sets))
    x, y = np.concatenate([a.ravel() for a in xs]), np.concatenate([a.ravel() for a in ys])

    def axis(v, cells):
        lo, hi = float(np.nanmin(v)), float(np.nanmax(v))
        pad = 0.1 * (hi - lo) + 1e-6
        return (lo - pad) + (hi - lo + 2 * pad) * (np.arange(cells + 1) / cells) ** 1.3
    kw = {}
    first = gate_sets[0]
    if 'echo_top' in products:
        kw['thresholds'] = {k: finite_quantiles(first[k], [0.3, 0.6]) if k != 'KDP' else finite_quantiles(first[k], [0.5]) for k in fields}
    if slab:
        kw['height_range'] = tuple(finite_quantiles(first['heights'], [0.05, 0.9]))
    return CP().Composite(fields, axis(x, n[0]), axis(y, n[1]), products=products, plane=plane, **kw)


def rule(spec, name, sweeps, rpb=0):
    """composite.compose over [(per-gate arrays, source)] in turn on the spec's plane, finished."""
    c = CP()
    state = None
    for gates, source in sweeps:
        state = c.compose(spec, {k: gates[k] for k in spec.fields}, None, gates['heights'], None, state=state, rays_per_block=rpb,
                          gate_xy=xy_of(spec.plane, gates, name), source=source)
    return c.finish(state)


# ---------------------------------------------------------------------------------------------------- one radar on a plane
@pytest.mark.parametrize('name', NAMES)
def test_geographic_plane_maps_of_the_rule_and_the_rest_of_the_call(name):
    op = op_for(name, 0)
    az, el = rays(name)
    plain, forms = plain_run(name, 0)
    spec = spec_on('geographic', name, [plain])
    assert spec.x_edges[0] < 7.5 and 45.0 < spec.y_edges[0] < 47.0                # (degrees: longitudes east, latitudes north)
    res = op.simulate_rays_composite(az, el, spec, keep_gates=True)
    got, gates = maps_of(res), arrays(res)
    assert op._ctx.launch_forms() == forms
    for k, v in plain.items():                           # the per-gate arrays are those of the call without the composite
        assert same_gates(gates[k], v), ('per-gate', k)
    assert_maps(got, rule(spec, name, [(gates, 0)]), spec, name + '/geographic')   # (asserts >= 3 occupied cells, >= 1 empty)
    only = op.simulate_rays_composite(az, el, spec)
    assert 'ZH' not in only and 'mask' not in only
    assert_maps(maps_of(only), got, spec, name + '/maps only')
    per_ray = op.simulate_rays_composite(az, el, spec, keep_gates=True, rays_per_block=1)
    assert_maps(maps_of(per_ray), rule(spec, name, [(arrays(per_ray), 0)], rpb=1), spec, name + '/per ray', not_empty=False)


def test_stencils_and_forms_are_left_alone_and_the_third_repeat_replays():
    """Five plain sweeps of a geometry on one fresh operator; on another four composite calls on the geographic plane, the first
    of which fetches the gate coordinates of the geometry by ONE plain call of its own: the device sees the same five sweeps, so
    composite call i leaves the stencil form and the launch forms of plain sweep i + 1, and its per-gate arrays are that sweep's."""
    name = 'c2_rsg'
    conf, luts, cubes, _, _ = case(name)
    az, el = rays(name)
    spec = spec_on('geographic', name, [plain_run(name, 0)[0]])
    seen = {}
    for with_comp in (False, True):
        op = operator(conf, luts)
        load(op, cubes[0])
        st, forms, out = [], [], []
        for i in range(4 if with_comp else 5):
            res = op.simulate_rays_composite(az, el, spec, keep_gates=True) if with_comp else op.simulate_rays(az, el)
            out.append((arrays(res), maps_of(res) if with_comp else None))
            st.append(op.stencil_state()['form'])
            forms.append(op._ctx.launch_forms())
        if with_comp:
            assert op._ctx.composite_plane() == (1, 3)
        seen[with_comp] = (st, forms, out)
        op.close()
    print('stencil forms without / with the composite:', seen[False][0], seen[True][0])
    assert seen[False][0][1:] == seen[True][0] and seen[True][0][2] == 2 and seen[True][0][-1] == 2
    assert seen[False][1][1:] == seen[True][1]
    for i in range(4):
        for k, v in seen[False][2][i + 1][0].items():
            assert same_gates(seen[True][2][i][0][k], v), (i, k)
        assert_maps(seen[True][2][i][1], rule(spec, name, [(seen[True][2][i][0], 0)]), spec, 'sweep %d' % i)


def test_repeat_calls_upload_the_plane_once():
    name = 'c4_7x7'
    op = op_for(name, 0)
    az, el = rays(name, shift=0.25)                      # (a geometry no other test of this module has shown the operator)
    plain = arrays(op.simulate_rays(az, el))
    spec = spec_on('geographic', name, [plain], products=('max', 'lowest'), slab=False)
    up0, hit0 = op._ctx.composite_plane()
    maps, stats = [], []
    for i in range(3):
        maps.append(maps_of(op.simulate_rays_composite(az, el, spec)))
        stats.append(op._ctx.composite_plane())
    assert stats == [(up0 + 1, hit0), (up0 + 1, hit0 + 1), (up0 + 1, hit0 + 2)], (up0, hit0, stats)
    assert_maps(maps[0], rule(spec, name, [(plain, 0)]), spec, 'first call')
    for m in maps[1:]:
        assert_maps(m, maps[0], spec, 'repeat')
    # the plane coordinates are cached beside the geometry, read-only, and handed over as they are
    (key,) = [k for k in op._cache if isinstance(k, tuple) and len(k) == 5 and k[0] == 'plane' and k[3] == 'geographic'
              and np.array_equal(op._cache[k][1], plain['lons'])]
    tag, x, y = op._cache[key]
    assert tag > 0 and not x.flags.writeable and not y.flags.writeable and np.array_equal(y, plain['lats'])
    # another plane over the same geometry is another entry and another upload
    other = spec_on(local_metres, name, [plain], products=('max',), slab=False)
    got = maps_of(op.simulate_rays_composite(az, el, other))
    assert op._ctx.composite_plane() == (up0 + 2, hit0 + 2)
    assert_maps(got, rule(other, name, [(plain, 0)]), other, 'a callable plane')


@pytest.mark.parametrize('plane', ['model', 'callable'])
def test_other_planes(plane):
    name = 'c2_rsg'
    op = op_for(name, 0)
    az, el = rays(name)
    plain, _ = plain_run(name, 0)
    spec = spec_on('model' if plane == 'model' else local_metres, name, [plain])
    if plane == 'model':
        # rotated degrees of the model's own grid: the gates lie inside the cube's rotated box
        p = case(name)[2][0]['proj_info']
        assert p['Lo1'] < spec.x_edges[1] and spec.x_edges[-2] < p['Lo2'] and p['La1'] < spec.y_edges[1] and spec.y_edges[-2] < p['La2']
    else:
        assert spec.x_edges[-1] - spec.x_edges[0] > 1e3                         # metres
    res = op.simulate_rays_composite(az, el, spec, keep_gates=True)
    assert_maps(maps_of(res), rule(spec, name, [(arrays(res), 0)]), spec, name + '/' + plane)


# ---------------------------------------------------------------------------------------------------- two radars
@functools.lru_cache(maxsize=None)
def network(name):
    """(operator, az, elevations, radars, the per-gate arrays [radar][elevation], the spec): the second radar is the first moved
    10 km down its own beam (gate 33 of the middle ray: the cube reaches 61 km from the first radar, the rays 45 km from either),
    so the two cover overlapping stretches of one line."""
    op = op_for(name, 0)
    az, el = rays(name)
    conf = case(name)[0]
    first = [float(v) for v in conf['radar']['coords']]
    plain, _ = plain_run(name, 0)
    second = [float(plain['lats'][3, 33]), float(plain['lons'][3, 33]), first[2]]
    radars = [first, second]
    elevations = [float(el[0]), float(el[0]) + 1.5]
    spec0 = CP().Composite('ZH', [0.0, 1.0], [0.0, 1.0], plane='geographic')
    gates = [[arrays(op.simulate_rays_composite(az, np.full(len(az), e), spec0, keep_gates=True, radar=r)) for e in elevations] for r in radars]
    spec = spec_on('geographic', name, [g for per in gates for g in per], products=('max', 'lowest', 'echo_top', 'source'), slab=False)
    return op, az, elevations, radars, gates, spec


@pytest.mark.parametrize('name', NAMES)
def test_two_radars_placing_the_second(name):
    op, az, elevations, radars, gates, spec = network(name)
    # the second radar's sweep stays inside the cube: as many gates with a value as the first one's, within a tenth
    n = [[int(np.isfinite(g['ZH']).sum()) for g in per] for per in gates]
    print('gates with a value per radar and elevation:', n)
    assert min(n[1]) > 0.9 * min(n[0]) > 0
    assert not same_gates(gates[0][0]['lats'], gates[1][0]['lats']) and not same_gates(gates[0][0]['heights'], gates[1][0]['heights'])
    # from the rule, on the CPU: each radar owns a cell alone, and they share one
    alone = [rule(spec, name, [(g, 0) for g in per])['count']['ZH'][0] for per in gates]
    only_first, only_second, both = (alone[0] > 0) & (alone[1] == 0), (alone[1] > 0) & (alone[0] == 0), (alone[0] > 0) & (alone[1] > 0)
    print('cells of the first alone, of the second alone, shared:', int(only_first.sum()), int(only_second.sum()), int(both.sum()))
    assert only_first.any() and only_second.any() and both.any()


@pytest.mark.parametrize('name', NAMES)
def test_two_radars_fold_into_one_pass_with_their_sources(name):
    op, az, elevations, radars, gates, spec = network(name)
    res = op.get_network_composite(radars, elevations, spec, azimuths=az, keep_gates=True)
    assert sorted(res) == ['composite', 'sweeps'] and [len(per) for per in res['sweeps']] == [2, 2]
    for r in range(2):
        for e in range(2):
            for k, v in gates[r][e].items():             # every sweep's arrays are those of the radar's own call
                assert same_gates(np.array(res['sweeps'][r][e][k]), v), (r, e, k)
    got = maps_of(res)
    want = rule(spec, name, [(gates[r][e], r) for r in range(2) for e in range(2)])
    assert_maps(got, want, spec, name + '/network')
    for p in ('source_of_max', 'source_of_lowest'):
        seen = got['values']['ZH'][p]
        assert set(np.unique(seen[~np.isnan(seen)]).tolist()) == {0.0, 1.0}, (p, seen)
        assert same(np.isnan(seen), np.isnan(got['values']['ZH']['max']))
    # the radars listed in the other order, the sources following: the same maps but for the sources
    back = maps_of(op.get_network_composite(radars[::-1], elevations, spec, azimuths=az))
    assert_maps(back, rule(spec, name, [(gates[r][e], 1 - r) for r in (1, 0) for e in range(2)]), spec, name + '/network reversed')
    for k in spec.fields:
        for p in spec.planes(k):
            if not p.startswith('source_of_'):
                assert same(back['values'][k][p], got['values'][k][p]), (k, p)
        assert same(back['count'][k], got['count'][k]), k
    assert not same(back['values']['ZH']['source_of_max'], got['values']['ZH']['source_of_max'])
    # without 'source' the pass is the same maps, and every call's source is 0
    plain_spec = spec_on('geographic', name, [g for per in gates for g in per], slab=False)
    plain = maps_of(op.get_network_composite(radars, elevations, plain_spec, azimuths=az))
    for k in plain_spec.fields:
        for p in plain_spec.planes(k):
            assert same(plain['values'][k][p], got['values'][k][p]), (k, p)


def test_network_refusals():
    name = 'c2_rsg'
    op, az, elevations, radars, gates, spec = network(name)
    radar_plane = CP().Composite('ZH', [-1e5, 0.0, 1e5], [-1e5, 0.0, 1e5])
    with pytest.raises(ValueError, match="plane 'radar' is centred on ONE radar"):
        op.get_network_composite(radars, elevations, radar_plane, azimuths=az)
    with pytest.raises(ValueError, match='at most 255'):
        op.get_network_composite([radars[0]] * 256, elevations, spec, azimuths=az)
    with pytest.raises(ValueError, match='three finite numbers'):
        op.get_network_composite([radars[0][:2]], elevations, spec, azimuths=az)
    with pytest.raises(ValueError, match='0 ... 254'):
        op.simulate_rays_composite(az, np.full(len(az), elevations[0]), spec, source=255)
    with pytest.raises(ValueError, match='non-zero source'):
        op.simulate_rays_composite(az, np.full(len(az), elevations[0]), radar_plane, source=1)
    # one radar on the radar plane through the network entry: get_PPI_composite's maps
    one = maps_of(op.get_network_composite(radars[:1], elevations, radar_plane, azimuths=az))
    ppi = maps_of(op.get_PPI_composite(elevations, radar_plane, azimuths=az))
    assert_maps(one, ppi, radar_plane, 'one radar', not_empty=False)
    assert int(one['count']['ZH'].sum()) > 0


def test_network_scores_equal_the_rule_of_the_returned_map():
    name = 'c2_rsg'
    op, az, elevations, radars, gates, spec = network(name)
    forecast = rule(spec, name, [(gates[r][e], r) for r in range(2) for e in range(2)])['values']['ZH']['max'][0]
    observed = np.roll(forecast, 1, axis=1)
    v = np.sort(forecast[np.isfinite(forecast)].astype(np.float64))
    fr = NB().Fractions(spec, 'ZH', [float(v[int(q * (v.size - 1))]) for q in (0.25, 0.5, 0.75)], [0, 1, 3])
    res = op.get_network_composite_fss(radars, elevations, fr, observed, azimuths=az)
    got = maps_of(res)
    assert same(got['values']['ZH']['max'][0], forecast)
    want = NB().sums(fr, got['values']['ZH']['max'], observed, None)
    for k in ('diff2', 'forecast2', 'observed2', 'n_forecast', 'n_observed', 'n_domain'):
        assert np.array_equal(np.array(res['composite']['fractions'][k]), want[k]), k
    assert want['forecast2'].any() and want['observed2'].any() and want['diff2'].any()
    assert all('composite' not in sw for per in res['sweeps'] for sw in per)          # scored once, at the end of the pass
    with pytest.raises(ValueError, match='not a plane to score'):
        NB().Fractions(spec, 'ZH', [1.0], [1], plane='source_of_max')


def test_ensemble_on_the_geographic_plane_per_member():
    name = 'c4_7x7'
    op, _, _ = E.ensemble_operator(name)
    az, el = rays(name)
    first = arrays(op.simulate_rays_ensemble(az, el))
    geo = dict(first, **{k: np.array(v) for k, v in op.simulate_rays(az, el).items() if k in ('lats', 'lons')})
    spec = spec_on('geographic', name, [dict(geo, **{k: first[k][0] for k in FIELDS})], products=('max', 'lowest', 'source'), slab=False)
    kept = op.simulate_rays_ensemble_composite(az, el, spec, keep_gates=True, source=4)
    got, gates = maps_of(kept), arrays(kept)
    assert got['count']['ZH'].shape[0] == 3
    assert_maps(got, rule(spec, name, [(gates, 4)], rpb=len(az)), spec, 'ensemble on the geographic plane')
    seen = got['values']['ZH']['source_of_max']
    assert set(np.unique(seen[~np.isnan(seen)]).tolist()) == {4.0}
    for m in range(3):
        op.select_member(m)
        alone = maps_of(op.simulate_rays_composite(az, el, spec, source=4))
        for k in spec.fields:
            for q in spec.planes(k):
                assert same(got['values'][k][q][m:m + 1], alone['values'][k][q]), (m, k, q)
    op.select_member(0)
    assert not same(got['values']['ZH']['max'][0], got['values']['ZH']['max'][1])
    op.close()


def test_time_blend_on_the_geographic_plane_with_a_moved_radar():
    import test_gpu_timed as T
    name = 'c4_7x7'
    op, _, _ = T.series_operator(name)
    az, el = rays(name)
    plain = T.arrays(op.simulate_rays_at(az, el, 200.0))
    moved = [float(plain['lats'][3, 20]), float(plain['lons'][3, 20]), float(case(name)[0]['radar']['coords'][2])]
    spec = spec_on('geographic', name, [plain], products=('max', 'lowest', 'source'), slab=False, n=(12, 9))
    here = op.simulate_rays_at_composite(az, el, 200.0, spec, keep_gates=True, source=2)
    for k, v in plain.items():
        assert same_gates(arrays(here)[k], v), k
    assert_maps(maps_of(here), rule(spec, name, [(arrays(here), 2)]), spec, 'timed')
    # the radar moved for this call alone: other gate coordinates, the maps of the rule on them; the configuration's radar after it
    there = op.simulate_rays_at_composite(az, el, 200.0, spec, keep_gates=True, radar=moved, source=1)
    assert not same_gates(arrays(there)['lats'], plain['lats'])
    assert_maps(maps_of(there), rule(spec, name, [(arrays(there), 1)]), spec, 'timed, moved', not_empty=False)
    assert int(maps_of(there)['count']['ZH'].sum()) > 0
    fr = NB().Fractions(spec, 'ZH', [float(np.nanmedian(maps_of(here)['values']['ZH']['max']))], [0, 1])
    scored = op.simulate_rays_at_composite_fss(az, el, 200.0, fr, maps_of(there)['values']['ZH']['max'][0], source=2)
    assert_maps(maps_of(scored), maps_of(here), spec, 'timed, scored')
    want = NB().sums(fr, maps_of(scored)['values']['ZH']['max'], maps_of(there)['values']['ZH']['max'][0], None)
    assert np.array_equal(np.array(scored['composite']['fractions']['diff2']), want['diff2'])
    op.close()
