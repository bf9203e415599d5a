"""Height layers and the column of the gridded composites on the GPU through the sweeps: the layered maps, the column and its
layer count of a call with keep_gates=True against composite.compose / composite.finish of that call's own per-gate arrays, bit
for bit (NaNs positionally equal), and the per-gate arrays against the same call without the composite.

One small operator (the golden radial c2_rsg, seven rays at az + 0.5 k), a 9 x 7 grid over the gates of a first plain call and
6 layers between quantiles of its heights, ZH with composite.vil_table() and KDP without a table."""
import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_composite_sweeps import maps_of, plain_run, same, same_gates, spec_for
from test_gpu_composite_network import network, pole_of, xy_of        # noqa: F401
from test_gpu_histogram_sweeps import arrays, op_for, rays, _ops

pytestmark = pytest.mark.gpu

NAME = 'c2_rsg'
FIELDS = ['ZH', 'KDP']


def CP():
    from cosmo_pol_amd import composite
    return composite


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def layers_of(heights, n=6):
    h = np.asarray(heights, dtype=np.float64).ravel()
    h = h[np.isfinite(h)]
    lo, hi = np.quantile(h, [0.02, 0.95])
    return lo + (hi - lo) * np.arange(n + 1) / n


def layered_like(base, heights, gaps='hold', plane=None):
    """The grid of `base` with 6 layers and the VIL of ZH."""
    return CP().Composite(FIELDS, base.x_edges, base.y_edges, products=('max', 'column'), z_edges=layers_of(heights),
                          column={'ZH': CP().vil_table()}, gaps=gaps, plane=base.plane if plane is None else plane)


def layered_spec(gaps='hold'):
    plain, _ = plain_run(NAME, 0)
    az, _ = rays(NAME)
    return layered_like(spec_for(plain, az, ('max',), False, FIELDS), plain['heights'], gaps)


def column_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def assert_layered(res, want, spec, tag, not_empty=True):
    got = res['composite']
    assert sorted(got) == ['column', 'column_layers', 'count', 'values', 'x_edges', 'y_edges', 'z_edges'], (tag, sorted(got))
    assert np.array_equal(got['z_edges'], spec.z_edges) and got['z_edges'].dtype == np.float32
    for k in spec.fields:
        assert list(got['values'][k]) == ['max', 'height_of_max'], (tag, k)
        for p in ('max', 'height_of_max'):
            assert same(np.array(got['values'][k][p]), want['values'][k][p]), (tag, k, p)
        assert same(np.array(got['count'][k]), want['count'][k]), (tag, k, 'count')
    assert list(got['column']) == ['ZH'] == list(got['column_layers'])
    col, lay = np.array(got['column']['ZH']), np.array(got['column_layers']['ZH'])
    assert column_bits(col, want['column']['ZH']), (tag, 'column', col, want['column']['ZH'])
    assert lay.dtype == np.uint8 and np.array_equal(lay, want['column_layers']['ZH']), (tag, 'column_layers')
    n = np.array(got['count']['ZH'])
    print('%s: %d gates counted in %d of %d (layer, cell)s; columns in %d cells, largest %.3g kg m-2, up to %d layers' % (
        tag, int(n.sum()), int((n > 0).sum()), n.size, int(np.isfinite(col).sum()), float(np.nanmax(col)) if np.isfinite(col).any() else 0.0, int(lay.max())))
    if not_empty:
        assert int((n > 0).sum()) >= 6 and int((n.sum(axis=1) == 0).sum()) >= 1 and np.nanmax(col) > 0.0, tag
        assert (n > 0).any(axis=(0, 2, 3)).sum() >= 3, (tag, 'layers with gates')


def rule(spec, sweeps, rpb=0, xy=None):
    c = CP()
    state = None
    for i, (gates, az) in enumerate(sweeps):
        if xy is None:
            state = c.compose(spec, {k: gates[k] for k in spec.fields}, gates['dist'], gates['heights'], az, state=state, rays_per_block=rpb)
        else:
            state = c.compose(spec, {k: gates[k] for k in spec.fields}, None, gates['heights'], None, state=state, rays_per_block=rpb, gate_xy=xy[i])
    return c.finish(state)


def test_one_sweep_and_a_volume_of_three():
    op = op_for(NAME, 0, lanes=2)
    az, el = rays(NAME)
    plain, forms = plain_run(NAME, 0)
    spec = layered_spec()
    res = op.simulate_rays_composite(az, el, spec, keep_gates=True)
    gates = arrays(res)
    assert op._ctx.launch_forms() == forms
    for k, v in plain.items():                           # the per-gate arrays are those of simulate_rays
        assert same_gates(gates[k], v), ('per-gate', k)
    assert_layered(res, rule(spec, [(gates, az)]), spec, 'one sweep')
    only = op.simulate_rays_composite(az, el, spec)
    assert 'ZH' not in only and 'mask' not in only
    assert_layered(only, rule(spec, [(gates, az)]), spec, 'one sweep, maps only')
    per_ray = op.simulate_rays_composite(az, el, spec, keep_gates=True, rays_per_block=1)
    assert np.array(per_ray['composite']['column']['ZH']).shape == (len(az), spec.n_y, spec.n_x)
    assert_layered(per_ray, rule(spec, [(arrays(per_ray), az)], rpb=1), spec, 'per ray', not_empty=False)
    # the other gaps rule: fewer layers, the same maps
    zero = layered_spec('zero')
    rz = op.simulate_rays_composite(az, el, zero, keep_gates=True)
    assert_layered(rz, rule(zero, [(arrays(rz), az)]), zero, 'gaps zero')
    assert (np.array(rz['composite']['column_layers']['ZH']) <= np.array(res['composite']['column_layers']['ZH'])).all()
    # three elevations fold into one pass
    elevations = [4.0, 5.0, 6.0]
    kept = op.get_PPI_composite(elevations, spec, azimuths=az, keep_gates=True)
    assert len(kept['sweeps']) == 3 and 'composite' not in kept['sweeps'][0]
    want = rule(spec, [(arrays(s), az) for s in kept['sweeps']])
    assert_layered(kept, want, spec, 'volume')
    for s, e in zip(kept['sweeps'], elevations):
        alone = arrays(op.simulate_rays(az, np.full(len(az), e)))
        for k in ('ZH', 'KDP', 'heights', 'dist'):
            assert same_gates(arrays(s)[k], alone[k]), (e, k)
    volume = op.get_PPI_composite(elevations, spec, azimuths=az)
    assert 'ZH' not in volume['sweeps'][0]
    assert_layered(volume, want, spec, 'volume, maps only')
    per_sweep = op.get_PPI_composite(elevations, spec, azimuths=az, per_sweep=True, keep_gates=True)
    assert len(per_sweep) == 3
    for i in range(3):
        assert_layered(per_sweep[i], rule(spec, [(arrays(per_sweep[i]), az)]), spec, 'sweep %d' % i, not_empty=False)
    # page-locked outputs, waited for
    lazy = op.simulate_rays_composite(az, el, spec, pinned=True)
    op.wait()
    assert_layered(lazy, rule(spec, [(gates, az)]), spec, 'pinned')


def test_device_outputs():
    """(Alone, this test also pays for torch's first use of the device in the session; its own four sweeps take milliseconds.)"""
    import torch
    op = op_for(NAME, 0, lanes=2)
    az, el = rays(NAME)
    spec = layered_spec()
    want = op.simulate_rays_composite(az, el, spec)['composite']
    sh = (1, spec.n_z, 2, spec.n_y, spec.n_x)
    dv = {k: torch.full(sh, 77.0, dtype=torch.float32, device='cuda') for k in spec.fields}
    dc = torch.full(sh, 77, dtype=torch.int64, device='cuda')
    col = torch.full((1, spec.n_y, spec.n_x), 77.0, dtype=torch.float64, device='cuda')
    lay = torch.full((1, spec.n_y, spec.n_x), 77, dtype=torch.uint8, device='cuda')
    ptrs = {'composite': {'values': {k: a.data_ptr() for k, a in dv.items()}, 'count': dc.data_ptr(), 'column': {'ZH': col.data_ptr()},
                          'column_layers': {'ZH': lay.data_ptr()}}}
    op.simulate_rays_composite(az, el, spec, phase=1, device_outputs=ptrs)
    op.wait()
    assert (col == 77.0).all().item() and (lay == 77).all().item() and (dc == 77).all().item()       # nothing is written before the finish
    op.simulate_rays_composite(az, el, spec, phase=2, device_outputs=ptrs)
    op.wait()
    # the same sweep twice: the maxima and the column are those of one, the counts double
    assert column_bits(col.cpu().numpy(), np.array(want['column']['ZH'])) and np.array_equal(lay.cpu().numpy(), np.array(want['column_layers']['ZH']))
    for i, k in enumerate(spec.fields):
        assert np.array_equal(dc.cpu().numpy().view(np.uint64)[:, :, i], 2 * np.array(want['count'][k])), k
        for j, q in enumerate(('max', 'height_of_max')):
            assert same(dv[k].cpu().numpy()[:, :, j], np.array(want['values'][k][q])), (k, q)


def test_ensemble_per_member():
    op, _, _ = E.ensemble_operator(NAME)
    az, el = rays(NAME)
    first = arrays(op.simulate_rays_ensemble(az, el))
    spec = layered_like(spec_for(first, az, ('max',), False, FIELDS), first['heights'])
    kept = op.simulate_rays_ensemble_composite(az, el, spec, keep_gates=True)
    gates = arrays(kept)
    n_members = gates['ZH'].shape[0]
    assert n_members >= 2 and gates['heights'].shape == gates['ZH'].shape[1:]
    for k in FIELDS:
        assert same_gates(gates[k], first[k]), k
    assert_layered(kept, rule(spec, [(gates, az)], rpb=len(az)), spec, 'ensemble')
    assert np.array(kept['composite']['column']['ZH']).shape == (n_members, spec.n_y, spec.n_x)
    whole = op.simulate_rays_ensemble_composite(az, el, spec, per_member=False)
    assert_layered(whole, rule(spec, [(gates, az)]), spec, 'ensemble, one map')
    # the member list cut into chunks: the blocks joined
    op.sequence_memory_budget = 1
    cut = op.simulate_rays_ensemble_composite(az, el, spec)
    op.sequence_memory_budget = None
    assert_layered(cut, rule(spec, [(gates, az)], rpb=len(az)), spec, 'ensemble in chunks')
    op.close()


def test_time_blend():
    import test_gpu_timed as T
    op, _, _ = T.series_operator(NAME)
    az, el = rays(NAME)
    plain = T.arrays(op.simulate_rays_at(az, el, 200.0))
    spec = layered_like(spec_for(plain, az, ('max',), False, FIELDS), plain['heights'])
    res = op.simulate_rays_at_composite(az, el, 200.0, spec, keep_gates=True)
    gates = arrays(res)
    for k, v in plain.items():
        assert same_gates(gates[k], v), k
    assert_layered(res, rule(spec, [(gates, az)]), spec, 'timed')
    op.close()


def test_two_radars_on_the_geographic_plane():
    # (the function behind the other module's cache: that cache would hand this module's operator, closed at its end, to the tests there)
    op, az, elevations, radars, gates, net = network.__wrapped__(NAME)
    flat = [g for per in gates for g in per]
    spec = layered_like(net, np.concatenate([g['heights'].ravel() for g in flat]), plane='geographic')
    res = op.get_network_composite(radars, elevations, spec, azimuths=az, keep_gates=True)
    assert [len(per) for per in res['sweeps']] == [2, 2]
    for r in range(2):
        for e in range(2):
            for k in ('ZH', 'KDP', 'heights', 'lats', 'lons'):
                assert same_gates(np.array(res['sweeps'][r][e][k]), gates[r][e][k]), (r, e, k)
    want = rule(spec, [(g, None) for g in flat], xy=[xy_of('geographic', g, NAME) for g in flat])
    assert_layered(res, want, spec, 'network')
    # each radar alone reaches fewer (layer, cell)s than both
    alone = [rule(spec, [(g, None) for g in per], xy=[xy_of('geographic', g, NAME) for g in per])['count']['ZH'] for per in gates]
    both = want['count']['ZH']
    assert ((alone[0] > 0).sum() < (both > 0).sum()) and ((alone[1] > 0).sum() < (both > 0).sum())
    # 'source' stays out of a layered pass
    with pytest.raises(ValueError, match="z_edges with 'source'"):
        CP().Composite(FIELDS, net.x_edges, net.y_edges, products=('max', 'source'), z_edges=[0.0, 1.0], plane='geographic')


def test_a_plain_spec_gives_what_it_gave_and_scores_beside_layers_are_refused():
    from cosmo_pol_amd import neighbourhood as NB
    op = op_for(NAME, 0)                                 # (the operator of plain_run: its launch forms are compared)
    az, el = rays(NAME)
    plain, forms = plain_run(NAME, 0)
    spec = layered_spec()
    base = spec_for(plain, az, ('max',), False, FIELDS)
    before = maps_of(op.simulate_rays_composite(az, el, base, keep_gates=True))
    op.simulate_rays_composite(az, el, spec)
    res = op.simulate_rays_composite(az, el, base, keep_gates=True)
    after = maps_of(res)
    assert sorted(res['composite']) == ['count', 'values', 'x_edges', 'y_edges'] and op._ctx.launch_forms() == forms
    want = CP().finish(CP().compose(base, {k: plain[k] for k in FIELDS}, plain['dist'], plain['heights'], az))
    for k in FIELDS:
        for p in ('max', 'height_of_max'):
            assert same(after['values'][k][p], before['values'][k][p]) and same(after['values'][k][p], want['values'][k][p]), (k, p)
        assert same(after['count'][k], before['count'][k]) and same(after['count'][k], want['count'][k]), k
    # the column maximum of the layered maps over the layers is the plain maximum wherever every counting gate lies in a layer
    lay = maps_of(op.simulate_rays_composite(az, el, spec))
    inside = lay['count']['ZH'].sum(axis=1) == after['count']['ZH']
    assert inside.any()
    with np.errstate(invalid='ignore'):
        top = np.fmax.reduce(lay['values']['ZH']['max'], axis=1)
    assert same(top[inside & (after['count']['ZH'] > 0)], after['values']['ZH']['max'][inside & (after['count']['ZH'] > 0)])
    # the library refuses scores beside layers (the Python layer refuses the spec itself; here its composite is swapped in behind it)
    with pytest.raises(ValueError, match='height layers is not scored'):
        NB.Fractions(spec, 'ZH', [1.0], [1])
    fr = NB.Fractions(base, 'ZH', [1.0], [1])
    fr.composite = spec
    with pytest.raises(ValueError, match='height layers is not scored'):
        op.simulate_rays_composite_fss(az, el, fr, np.zeros((spec.n_y, spec.n_x), np.float32))
    # ... and the context goes on
    again = maps_of(op.simulate_rays_composite(az, el, base))
    assert same(again['values']['ZH']['max'], before['values']['ZH']['max'])
