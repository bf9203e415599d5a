"""The exact sums of the composites on the GPU through the operator (the product 'sum'): `sum`, `sum_skipped` and every other
map of a call with keep_gates=True against composite.compose / composite.finish of that call's own per-gate arrays, bit for bit
(NaNs positionally equal) -- one sweep unweighted and under objects.zr_table, a volume of three elevations folded in one pass,
an ensemble per member against single calls, two radar sites on a geographic plane, page-locked and device-resident outputs, a scored call,
and composite.mean_of against its definition.  The cubes and grids are those of the sibling sweep tests."""
import numpy as np
import pytest

import test_gpu_ensemble as E
from test_composite_sums_cpu import same
from test_gpu_composite_network import rule as plane_rule, spec_on
from test_gpu_composite_sweeps import maps_of as plain_maps_of, plain_run, rule, spec_for
from test_gpu_ensemble import case
from test_gpu_histogram_sweeps import arrays, op_for, rays, _ops

pytestmark = pytest.mark.gpu


def CP():
    from cosmo_pol_amd import composite
    return composite


def OB():
    from cosmo_pol_amd import objects
    return objects


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def maps_of(res):
    w = res['composite']
    out = plain_maps_of(res)
    out['sum'] = {k: np.array(a) for k, a in w['sum'].items()}
    out['sum_skipped'] = {k: np.array(a) for k, a in w['sum_skipped'].items()}
    return out


def with_sum(spec, weight=None, fields=None):
    """`spec` with the product 'sum' beside its own, on the same grid."""
    c = CP()
    kw = {}
    if 'echo_top' in spec.products:
        kw['thresholds'] = {k: spec.thresholds_given[k] for k in (fields or spec.fields)}
    if spec.height_range is not None:
        kw['height_range'] = spec.height_range_given
    return c.Composite(fields or spec.fields, spec.x_edges, spec.y_edges, products=spec.products + ('sum',), plane=spec.plane, weight=weight, **kw)


def assert_maps(got, want, spec, tag, not_empty=True):
    assert sorted(got['sum']) == sorted(spec.fields) == sorted(got['sum_skipped']), tag
    for k in spec.fields:
        same(got['sum'][k], want['sum'][k], (tag, k, 'sum'))
        same(got['sum_skipped'][k], want['sum_skipped'][k], (tag, k, 'sum_skipped'))
        same(got['count'][k], want['count'][k], (tag, k, 'count'))
        for p in spec.planes(k):
            same(got['values'][k][p], want['values'][k][p], (tag, k, p))
    s = got['sum'][spec.fields[0]]
    print('%s: %d of %d cells hold a sum of %s' % (tag, int(np.isfinite(s).sum()), s.size, spec.fields[0]))
    if not_empty:
        assert int(np.isfinite(s).sum()) >= 3 and int(np.isnan(s).sum()) >= 1, (tag, s)


@pytest.mark.parametrize('name', ['c2_rsg', 'c4_7x7'])
def test_one_sweep_unweighted_and_under_the_rain_rate_table(name):
    c = CP()
    op = op_for(name, 0)
    az, el = rays(name)
    plain, forms = plain_run(name, 0)
    base = spec_for(plain, az, fields=['ZH', 'ZDR', 'KDP'])
    for tag, spec in (('unweighted', with_sum(base)), ('zr_table', with_sum(base, weight={'ZH': OB().zr_table()}))):
        res = op.simulate_rays_composite(az, el, spec, keep_gates=True)
        got, gates = maps_of(res), arrays(res)
        assert op._ctx.launch_forms() == forms, tag
        want = rule(spec, [(gates, az)])
        assert_maps(got, want, spec, '%s/%s' % (name, tag))
        # the maps a spec without 'sum' gives are the same maps
        without = plain_maps_of(op.simulate_rays_composite(az, el, base))
        for k in base.fields:
            same(without['count'][k], got['count'][k], k)
            for p in base.planes(k):
                same(without['values'][k][p], got['values'][k][p], (k, p))
        # mean_of against its definition, from the result of the call itself
        for k in spec.fields:
            mean = c.mean_of(res['composite'], k)
            n = got['count'][k].astype(np.int64) - got['sum_skipped'][k].astype(np.int64)
            assert mean.shape == n.shape and np.array_equal(np.isnan(mean), n == 0), k
            assert np.array_equal(mean[n > 0], got['sum'][k][n > 0] / n[n > 0].astype(np.float64)), k
        if tag == 'zr_table':
            # a rain rate: no cell below zero, and some rain somewhere
            rate = c.mean_of(res['composite'], 'ZH')
            assert np.nanmin(rate) >= 0.0 and np.nanmax(rate) > 0.0
        # per ray, and without the gates
        per_ray = op.simulate_rays_composite(az, el, spec, keep_gates=True, rays_per_block=1)
        assert_maps(maps_of(per_ray), rule(spec, [(arrays(per_ray), az)], rpb=1), spec, '%s/%s/per ray' % (name, tag), not_empty=False)
        assert_maps(maps_of(op.simulate_rays_composite(az, el, spec)), got, spec, '%s/%s/maps only' % (name, tag))


def test_a_volume_of_three_elevations_in_one_pass():
    name = 'c2_rsg'
    op = op_for(name, 0, lanes=2)
    az, _ = rays(name)
    elevations = [4.0, 5.0, 6.0]
    spec = with_sum(spec_for(plain_run(name, 0)[0], az, fields=['ZH', 'KDP']), weight={'ZH': OB().zr_table()})
    kept = op.get_PPI_composite(elevations, spec, azimuths=az, keep_gates=True)
    want = rule(spec, [(arrays(s), az) for s in kept['sweeps']])
    assert_maps(maps_of(kept), want, spec, 'volume')
    # cut differently and in another order: the same bits
    op.simulate_rays_composite(az, np.full(len(az), 6.0), spec, phase=1)
    op.simulate_rays_composite(az, np.full(len(az), 4.0), spec, phase=0)
    last = op.simulate_rays_composite(az, np.full(len(az), 5.0), spec, phase=2)
    assert_maps(maps_of(last), want, spec, 'volume in another order')
    one = maps_of(op.simulate_rays_composite(az, np.full(len(az), 4.0), spec))
    assert not np.array_equal(one['count']['ZH'], want['count']['ZH'])


def test_ensemble_of_three_members_against_three_single_calls():
    name = 'c4_7x7'
    op, _, _ = E.ensemble_operator(name)
    az, el = rays(name)
    first = arrays(op.simulate_rays_ensemble(az, el))
    spec = with_sum(spec_for(first, az, fields=['ZH', 'ZV']), weight={'ZH': OB().zr_table()})
    kept = op.simulate_rays_ensemble_composite(az, el, spec, keep_gates=True)
    got, gates = maps_of(kept), arrays(kept)
    assert got['sum']['ZH'].shape[0] == 3 == got['sum_skipped']['ZV'].shape[0]
    assert_maps(got, rule(spec, [(gates, az)], rpb=len(az)), spec, 'ensemble')
    whole = maps_of(op.simulate_rays_ensemble_composite(az, el, spec, per_member=False))
    assert_maps(whole, rule(spec, [(gates, az)]), spec, 'ensemble, one map')
    for m in range(3):
        op.select_member(m)
        alone = maps_of(op.simulate_rays_composite(az, el, spec))
        for k in spec.fields:
            same(got['sum'][k][m:m + 1], alone['sum'][k], (m, k))
            same(got['sum_skipped'][k][m:m + 1], alone['sum_skipped'][k], (m, k))
    op.select_member(0)
    assert not np.array_equal(got['sum']['ZH'][0], got['sum']['ZH'][1], equal_nan=True)
    # the member list cut into chunks: the same maps
    op.sequence_memory_budget = 1
    cut = op.simulate_rays_ensemble_composite(az, el, spec)
    cut_whole = op.simulate_rays_ensemble_composite(az, el, spec, per_member=False)
    op.sequence_memory_budget = None
    assert_maps(maps_of(cut), got, spec, 'ensemble in chunks')
    assert_maps(maps_of(cut_whole), whole, spec, 'ensemble in chunks, one map')
    op.close()


def test_two_radar_sites_on_a_geographic_plane():
    name = 'c2_rsg'
    # the second radar is the first moved 10 km down its own beam, as in test_gpu_composite_network.network
    op = op_for(name, 0)
    az, el = rays(name)
    first = [float(v) for v in case(name)[0]['radar']['coords']]
    plain, _ = plain_run(name, 0)
    radars = [first, [float(plain['lats'][3, 33]), float(plain['lons'][3, 33]), first[2]]]
    elevations = [float(el[0]), float(el[0]) + 1.5]
    spec0 = CP().Composite('ZH', [0.0, 1.0], [0.0, 1.0], plane='geographic')
    gates = [[arrays(op.simulate_rays_composite(az, np.full(len(az), e), spec0, keep_gates=True, radar=r)) for e in elevations] for r in radars]
    spec = with_sum(spec_on('geographic', name, [g for per in gates for g in per], products=('max', 'lowest'), slab=False, fields=['ZH', 'KDP']),
                    weight={'ZH': OB().zr_table()})
    res = op.get_network_composite(radars, elevations, spec, azimuths=az, keep_gates=True)
    got = maps_of(res)
    want = plane_rule(spec, name, [(gates[r][e], 0) for r in range(2) for e in range(2)])
    assert_maps(got, want, spec, 'network')
    back = maps_of(op.get_network_composite(radars[::-1], elevations, spec, azimuths=az))
    assert_maps(back, got, spec, 'network reversed')
    alone = maps_of(op.get_network_composite(radars[:1], elevations, spec, azimuths=az))
    assert not np.array_equal(alone['sum']['ZH'], got['sum']['ZH'], equal_nan=True)


def test_page_locked_and_device_resident_outputs():
    import torch
    name = 'c2_rsg'
    op = op_for(name, 0)
    az, el = rays(name)
    spec = with_sum(spec_for(plain_run(name, 0)[0], az, fields=['ZH', 'ATT_H']), weight={'ZH': OB().zr_table()})
    locked = op.simulate_rays_composite(az, el, spec, keep_gates=True)
    want = maps_of(locked)
    assert_maps(want, rule(spec, [(arrays(locked), az)]), spec, 'page-locked, waited for')
    lazy = op.simulate_rays_composite(az, el, spec, pinned=True)
    op.wait()
    assert_maps(maps_of(lazy), want, spec, 'pinned')
    # device pointers through the operator, a pass of two calls: the integer sums of the same sweep twice double exactly
    sh = want['count']['ZH'].shape
    dv = {k: torch.full((sh[0], len(spec.planes(k))) + sh[1:], 77.0, dtype=torch.float32, device='cuda') for k in spec.fields}
    dc = torch.full((sh[0], len(spec.fields)) + sh[1:], 77, dtype=torch.int64, device='cuda')
    ds = {k: torch.full(sh, 77.0, dtype=torch.float64, device='cuda') for k in spec.fields}
    dk = {k: torch.full(sh, 77, dtype=torch.int32, device='cuda') for k in spec.fields}
    ptrs = {'composite': {'values': {k: a.data_ptr() for k, a in dv.items()}, 'count': dc.data_ptr(),
                          'sum': {k: a.data_ptr() for k, a in ds.items()}, 'sum_skipped': {k: a.data_ptr() for k, a in dk.items()}}}
    op.simulate_rays_composite(az, el, spec, phase=1, device_outputs=ptrs)
    op.wait()
    assert all((a == 77.0).all().item() for a in ds.values()) and all((a == 77).all().item() for a in dk.values())    # nothing before the finish
    op.simulate_rays_composite(az, el, spec, phase=2, device_outputs=ptrs)
    op.wait()
    for i, k in enumerate(spec.fields):
        same(dc.cpu().numpy().view(np.uint64)[:, i], 2 * want['count'][k], k)
        same(ds[k].cpu().numpy(), 2.0 * want['sum'][k], k)
        same(dk[k].cpu().numpy().view(np.uint32), 2 * want['sum_skipped'][k], k)
        for j, q in enumerate(spec.planes(k)):
            same(dv[k].cpu().numpy()[:, j], want['values'][k][q], (k, q))


def test_the_scored_call_takes_the_spec_unchanged():
    """simulate_rays_composite_fss over a spec with 'sum': the scores are those of the spec without it (the scored plane cannot be
    the sum), and the sums those of the unscored call."""
    from cosmo_pol_amd import neighbourhood as NB
    from test_gpu_neighbourhood_sweeps import KEYS, RADII, values_of
    name = 'c2_rsg'
    op = op_for(name, 0)
    az, el = rays(name)
    base = spec_for(plain_run(name, 0)[0], az, products=('max', 'lowest'), slab=False, fields=['ZH', 'KDP'], n=(23, 17))
    spec = with_sum(base, weight={'ZH': OB().zr_table()})
    unscored = maps_of(op.simulate_rays_composite(az, el, spec))
    forecast = unscored['values']['ZH']['max'][0]
    observed = np.array(op_for(name, 1).simulate_rays_composite(az, el, base)['composite']['values']['ZH']['max'][0])
    thresholds = values_of(forecast)
    scored = op.simulate_rays_composite_fss(az, el, NB.Fractions(spec, 'ZH', thresholds, RADII), observed)
    plain = op.simulate_rays_composite_fss(az, el, NB.Fractions(base, 'ZH', thresholds, RADII), observed)
    assert_maps(maps_of(scored), unscored, spec, 'scored')
    assert 'sum' not in plain['composite']
    for k in KEYS:
        assert np.array_equal(np.array(scored['composite']['fractions'][k]), np.array(plain['composite']['fractions'][k])), k
    assert np.array(scored['composite']['fractions']['forecast2']).any()
    with pytest.raises(ValueError):
        NB.Fractions(spec, 'ZH', thresholds, RADII, plane='sum')
