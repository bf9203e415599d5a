"""Object cells on the GPU through the sweeps (cpol_fractions.objects on a scored finishing call): the cells of a call against
objects.cells of the maps THE SAME CALL returns, np.array_equal, its scores against neighbourhood.sums as before.  The small
operator case of tests/test_gpu_neighbourhood_sweeps.py: the observed map is the composite of the case's second cube, the
thresholds are values of the forecast map itself.  The rule is asserted to find objects in the forecast and in the observation,
and more row runs than objects, so no test passes on empty maps or on an idle kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_composite_sweeps import assert_maps, maps_of, same
from test_gpu_histogram_sweeps import op_for, _ops
import test_gpu_neighbourhood_sweeps as NS
from test_gpu_neighbourhood_sweeps import KEYS as SUMS, captured, scored

pytestmark = pytest.mark.gpu

f4, u1, u4, u8, i4 = np.float32, np.uint8, np.uint32, np.uint64, np.int32
KEYS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')
NAME = 'c2_rsg'


def OB():
    from cosmo_pol_amd import objects
    return objects


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


@functools.lru_cache(maxsize=None)
def setup(name):
    """The neighbourhood sweeps' case with operators of this module's own: that module closes its operators when it ends, and its
    cache would hand them out closed."""
    return NS.setup.__wrapped__(name)


def objects_spec(spec, **kw):
    kw.setdefault('connectivity', 8)
    kw.setdefault('max_objects', 64)
    return OB().Objects(spec, **kw)


def same_cells(got, want, tag):
    for part, g, w in (('blocks', got, want), ('observed', got['observed'], want['observed'])):
        for k in KEYS:
            assert np.array(g[k]).dtype == u4 and np.array_equal(np.array(g[k]), w[k]), (tag, part, k, np.array(g[k]).ravel()[:8], w[k].ravel()[:8])
        assert np.array(g['peak']).dtype == f4 and np.array_equal(np.array(g['peak']).view(u4), w['peak'].view(u4)), (tag, part, 'peak')
        assert ('labels' in g) == ('labels' in w), (tag, part)
        if 'labels' in w:
            assert np.array(g['labels']).dtype == i4 and np.array_equal(np.array(g['labels']), w['labels']), (tag, part, 'labels')
    assert (got['connectivity'], got['min_area']) == (want['connectivity'], want['min_area']) and np.array_equal(got['thresholds'], want['thresholds'])


def celled(res, ospec, observed, domain, tag, busy=True):
    """The cells and the scores of `res` against the rules applied to the maps `res` itself carries."""
    spec = ospec.fractions
    maps, want_sums = scored(res, spec, observed, domain, tag)
    plane = maps['values'][spec.field][spec.plane]
    want = OB().cells(ospec, plane, observed, domain)
    same_cells(res['composite']['objects'], want, tag)
    if busy:
        F, O, _, _ = OB().binary_maps(spec, plane, observed, domain)
        assert want['n_objects'].any() and want['observed']['n_objects'].any(), (tag, 'the rule finds no object')
        runs = sum(len(OB()._runs(b)[0]) for b in F.reshape((-1,) + observed.shape))
        assert runs > sum(OB().label(b, ospec.connectivity)[1] for b in F.reshape((-1,) + observed.shape)), (tag, 'no merge')
    if ospec.min_area == 1 and int(want['n_objects'].max()) <= ospec.max_objects:
        assert np.array_equal(want['area'].sum(axis=-1, dtype=u8), want_sums['n_forecast']), (tag, 'sum of areas')
    return maps, want


def test_single_sweep_blocks_of_rays_and_terms():
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    for kw in ({'connectivity': 4}, {'connectivity': 8}, {'connectivity': 8, 'min_area': 3}, {'connectivity': 4, 'max_objects': 2},
               {'connectivity': 8, 'labels': False}):
        ospec = objects_spec(spec, **kw)
        res = op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain)
        _, want = celled(res, ospec, observed, domain, (NAME, sorted(kw.items())))
        assert want['n_objects'].shape == (1, 4) and want['first'].shape == (1, 4, ospec.max_objects)
    ospec = objects_spec(spec)
    res = op.simulate_rays_composite_fss(az, el, ospec, observed)                      # (NULL domain: every cell)
    celled(res, ospec, observed, None, 'no domain')
    per_ray = op.simulate_rays_composite_fss(az, el, ospec, observed, rays_per_block=1)
    _, want = celled(per_ray, ospec, observed, None, 'a block per ray')
    assert want['n_objects'].shape == (len(az), 4) and want['labels'].shape == (len(az), 4) + observed.shape
    assert want['observed']['n_objects'].shape == (4,)


def test_a_plain_fractions_returns_what_it_returned():
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    with_cells, seen_c = captured(op, lambda: op.simulate_rays_composite_fss(az, el, objects_spec(spec), observed, domain=domain))
    plain, seen_p = captured(op, lambda: op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain))
    assert 'objects' in with_cells['composite'] and 'objects' not in plain['composite']
    assert seen_c['slots'] == seen_p['slots'] == (True, True)
    assert_maps(maps_of(plain), maps_of(with_cells), cspec, 'plain against celled')
    for k in SUMS:
        assert np.array_equal(np.array(plain['composite']['fractions'][k]), np.array(with_cells['composite']['fractions'][k])), k
    scored(plain, spec, observed, domain, 'plain behind a celled call', skilful=True)


def direct(op, ospec, az, p, t, observed, domain, change=None):
    """One blocking cpol_run_sweep (outputs_on_device 0) with plain host arrays -> (maps, scores, cells)."""
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import composite as CP
    from cosmo_pol_amd import neighbourhood as NB
    spec = ospec.fractions
    cspec = spec.composite
    c, keep = N.Context.composite_struct(cspec, phase=3, azimuths=az)
    vals = {k: np.full((1, len(cspec.planes(k)), cspec.n_y, cspec.n_x), 77.0, f4) for k in cspec.fields}
    cnt = np.full((1, len(cspec.fields), cspec.n_y, cspec.n_x), 77, u8)
    for k in cspec.fields:
        c.values[CP.FIELDS.index(k)] = vals[k].ctypes.data
    c.count = cnt.ctypes.data
    f, _ = N.Context.fractions_struct(spec)
    nt = len(spec.thresholds)
    s, tt = np.full((1, nt, len(spec.radii), 3), 77, u8), np.full((1, nt, 3), 77, u8)
    obs, dom = np.ascontiguousarray(observed), np.ascontiguousarray(domain)
    f.observed, f.domain, f.sums, f.totals = obs.ctypes.data, dom.ctypes.data, s.ctypes.data, tt.ctypes.data
    o, okeep = N.Context.objects_struct(ospec, f)
    n = np.full((2, nt), 77, u4)
    table = np.full((2, nt, ospec.max_objects, 10), 77, u4)
    labels = np.full((2, nt, cspec.n_y, cspec.n_x), 77, i4)
    o.n_objects, o.table, o.labels = n.ctypes.data, table.ctypes.data, labels.ctypes.data
    if change:
        change(o)
    out = N.Outputs()
    out.composite, out.fractions = C.pointer(c), C.pointer(f)
    q = N.SweepParams.from_buffer_copy(p)
    q.outputs_on_device = 0
    op._ctx.run_sweep(q, t, out)
    op.wait()
    del keep, okeep
    maps = {'values': {k: {p_: vals[k][:, j] for j, p_ in enumerate(cspec.planes(k))} for k in cspec.fields},
            'count': {k: cnt[:, i] for i, k in enumerate(cspec.fields)}}
    return maps, NB.result(spec, s, tt), OB().result(ospec, n, table, labels)


def test_output_modes_and_refusals():
    """Page-locked buffers (waited for, and pinned=True + wait), blocking host buffers and device pointers carry the same cells;
    every refusal of the library is followed by a good call."""
    import torch
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = objects_spec(spec)
    locked, seen = captured(op, lambda: op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain))
    good, want = celled(locked, ospec, observed, domain, 'page-locked')
    want_sums = locked['composite']['fractions']
    lazy = op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain, pinned=True)
    op.wait()
    same_cells(lazy['composite']['objects'], want, 'pinned')
    maps, sums, got = direct(op, ospec, az, seen['p'], seen['t'], observed, domain)
    assert_maps(maps, good, cspec, 'blocking')
    same_cells(got, want, 'blocking')
    for word, change in (('connectivity must be 4 or 8', lambda o: setattr(o, 'connectivity', 5)),
                         ('min_area must be at least 1', lambda o: setattr(o, 'min_area', 0)),
                         ('max_objects must lie in', lambda o: setattr(o, 'max_objects', 0)),
                         ('max_objects must lie in', lambda o: setattr(o, 'max_objects', 65536)),
                         ('n_objects or table is NULL', lambda o: setattr(o, 'n_objects', None)),
                         ('n_objects or table is NULL', lambda o: setattr(o, 'table', None)),
                         ('table must be 8-byte aligned', lambda o: setattr(o, 'table', o.table + 4))):
        with pytest.raises(ValueError, match='cpol_objects: ' + word):
            direct(op, ospec, az, seen['p'], seen['t'], observed, domain, change=change)
        maps, sums, got = direct(op, ospec, az, seen['p'], seen['t'], observed, domain)
        same_cells(got, want, ('after the refusal', word))
        for k in SUMS:
            assert np.array_equal(sums[k], np.array(want_sums[k])), (word, k)
    _, _, got = direct(op, ospec, az, seen['p'], seen['t'], observed, domain, change=lambda o: setattr(o, 'labels', None))
    assert (got['labels'] == 77).all() and np.array_equal(got['area'], want['area'])       # (NULL labels: none written)
    # device outputs: everything is a device pointer; a pass of two calls writes nothing before its finish
    nt = len(spec.thresholds)
    dv = {k: torch.full((1, len(cspec.planes(k)), cspec.n_y, cspec.n_x), 77.0, dtype=torch.float32, device='cuda') for k in cspec.fields}
    dc = torch.full((1, len(cspec.fields), cspec.n_y, cspec.n_x), 77, dtype=torch.int64, device='cuda')
    ds = torch.full((1, nt, len(spec.radii), 3), 77, dtype=torch.int64, device='cuda')
    dt = torch.full((1, nt, 3), 77, dtype=torch.int64, device='cuda')
    dn = torch.full((2, nt), 77, dtype=torch.int32, device='cuda')
    dtab = torch.full((2, nt, ospec.max_objects, 10), 77, dtype=torch.int32, device='cuda')
    dl = torch.full((2, nt, cspec.n_y, cspec.n_x), 77, dtype=torch.int32, device='cuda')
    d_obs, d_dom = torch.from_numpy(observed).cuda(), torch.from_numpy(domain).cuda()
    entry = {'values': {k: a.data_ptr() for k, a in dv.items()}, 'count': dc.data_ptr(), 'observed': d_obs.data_ptr(),
             'domain': d_dom.data_ptr(), 'sums': ds.data_ptr(), 'totals': dt.data_ptr(), 'n_objects': dn.data_ptr(),
             'table': dtab.data_ptr(), 'labels': dl.data_ptr()}
    op.simulate_rays_composite_fss(az, el, ospec, None, phase=1, device_outputs={'composite': entry})
    op.wait()
    assert (dn == 77).all().item() and (dtab == 77).all().item() and (dl == 77).all().item()
    op.simulate_rays_composite_fss(az, el, ospec, None, phase=2, device_outputs={'composite': entry})
    op.wait()
    # (the same sweep folded twice: maxima and minima are those of one, so the plane and its cells are, too)
    assert same(dv['ZH'].cpu().numpy()[:, 0], good['values']['ZH']['max'])
    same_cells(OB().result(ospec, dn.cpu().numpy().view(u4), dtab.cpu().numpy().view(u4), dl.cpu().numpy()), want, 'device')
    # the operator's own refusals
    with pytest.raises(ValueError, match='neighbourhood.Fractions'):
        op.simulate_rays_composite_fss(az, el, cspec, observed)
    with pytest.raises(ValueError, match='connectivity must be 4 or 8'):
        objects_spec(spec, connectivity=6)
    celled(op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain), ospec, observed, domain, 'after the operator refusals')


def test_three_call_pass_and_folded_volume():
    """A pass cut into three calls is labelled only at its end; get_PPI_composite_fss folds the volume and labels it once."""
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = objects_spec(spec)
    whole = op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain)
    good, want = celled(whole, ospec, observed, domain, 'one call')
    parts = []
    for rows, phase in ((slice(0, 3), 1), (slice(3, 5), 0), (slice(5, 7), 2)):
        res, seen = captured(op, lambda: op.simulate_rays_composite_fss(az[rows], el[rows], ospec, observed, domain=domain, phase=phase))
        assert seen['slots'] == (True, phase == 2)
        parts.append(res)
    assert 'composite' not in parts[0] and 'composite' not in parts[1]
    assert_maps(maps_of(parts[2]), good, cspec, 'three calls')
    same_cells(parts[2]['composite']['objects'], want, 'three calls')
    op2 = op_for(NAME, 0, lanes=2)
    volume = op2.get_PPI_composite_fss([4.0, 5.0, 6.0], ospec, observed, domain=domain, azimuths=az)
    assert len(volume['sweeps']) == 3 and all('composite' not in s for s in volume['sweeps'])
    celled(volume, ospec, observed, domain, 'volume')
    per_sweep = op2.get_PPI_composite_fss([4.0, 6.0], ospec, observed, azimuths=az, per_sweep=True)
    wants = [celled(per_sweep[i], ospec, observed, None, 'sweep %d' % i)[1] for i in range(2)]
    assert not np.array_equal(wants[0]['labels'], wants[1]['labels'])


def test_time_blend():
    import test_gpu_timed as T
    op, _, _ = T.series_operator(NAME)
    _, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = objects_spec(spec, connectivity=4)
    celled(op.simulate_rays_at_composite_fss(az, el, 200.0, ospec, observed, domain=domain), ospec, observed, domain, 'timed')
    op.close()


def test_ensemble_per_member_in_one_chunk_and_one_chunk_per_member():
    op, _, _ = E.ensemble_operator(NAME)
    _, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = objects_spec(spec)
    got = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain)
    maps, want = celled(got, ospec, observed, domain, 'ensemble')
    assert want['n_objects'].shape == (3, 4) and want['labels'].shape == (3, 4) + observed.shape
    assert not np.array_equal(want['labels'][0], want['labels'][1])
    op.select_member(1)
    alone = op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain)['composite']['objects']
    for k in KEYS + ('labels',):
        assert np.array_equal(np.array(alone[k]), want[k][1:2]), k
    op.select_member(0)
    op.sequence_memory_budget = 1
    cut = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain)
    cut_whole = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain, per_member=False)
    op.sequence_memory_budget = None
    same_cells(cut['composite']['objects'], want, 'ensemble in chunks')
    whole = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain, per_member=False)
    _, ww = celled(whole, ospec, observed, domain, 'ensemble, one map')
    assert ww['n_objects'].shape == (1, 4)
    same_cells(cut_whole['composite']['objects'], ww, 'ensemble in chunks, one map')
    op.close()


def test_network():
    from test_gpu_composite_network import network, rule
    from cosmo_pol_amd import neighbourhood as NB
    op, az, elevations, radars, gates, spec = network.__wrapped__(NAME)        # (not the cached one: its operator is closed)
    forecast = rule(spec, NAME, [(gates[r][e], r) for r in range(2) for e in range(2)])['values']['ZH']['max'][0]
    observed = np.roll(forecast, 1, axis=1)
    v = np.sort(forecast[np.isfinite(forecast)].astype(np.float64))
    fr = NB.Fractions(spec, 'ZH', [float(v[int(q * (v.size - 1))]) for q in (0.25, 0.5, 0.75)], [0])
    ospec = OB().Objects(fr, connectivity=8, max_objects=32)
    res = op.get_network_composite_fss(radars, elevations, ospec, observed, azimuths=az)
    got = maps_of(res)
    assert same(got['values']['ZH']['max'][0], forecast)
    want = OB().cells(ospec, got['values']['ZH']['max'], observed, None)
    assert want['n_objects'].any() and want['observed']['n_objects'].any()
    same_cells(res['composite']['objects'], want, 'network')
    assert all('composite' not in sw for per in res['sweeps'] for sw in per)          # labelled once, at the end of the pass
    plain = op.get_network_composite_fss(radars, elevations, fr, observed, azimuths=az)
    assert 'objects' not in plain['composite']
    for k in SUMS:
        assert np.array_equal(np.array(plain['composite']['fractions'][k]), np.array(res['composite']['fractions'][k])), k
