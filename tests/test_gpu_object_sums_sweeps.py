"""The exact sums of the object cells on the GPU through the sweeps (cpol_objects.sums on a scored finishing call): the sums of a
call against objects.cells of the maps THE SAME CALL returns, on the bits; `sal` on the result.  The small operator case of
tests/test_gpu_objects_sweeps.py: the observed map is the composite of the case's second cube, the thresholds are values of the
forecast map itself.  The rule is asserted to find objects with a volume in the forecast and in the observation, so no test
passes on empty maps or on an idle kernel."""
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_composite_sweeps import maps_of, same
from test_gpu_histogram_sweeps import _ops
import test_gpu_neighbourhood_sweeps as NS

pytestmark = pytest.mark.gpu

f4, f8, u1, u4, u8, i4 = np.float32, np.float64, np.uint8, np.uint32, np.uint64, np.int32
INTS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell', 'skipped')
FLOATS = ('volume', 'moment_x', 'moment_y')
NEW = {'volume', 'moment_x', 'moment_y', 'skipped', 'field'}
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
    """The neighbourhood sweeps' case with operators of this module's own (that module closes its operators when it ends)."""
    return NS.setup.__wrapped__(name)


def bits(a):
    a = np.ascontiguousarray(np.array(a))
    return a.view({4: u4, 8: u8}[a.dtype.itemsize])


def same_sums(got, want, tag):
    for part, g, w in (('blocks', got, want), ('observed', got['observed'], want['observed'])):
        for k in INTS:
            assert np.array(g[k]).dtype == u4 and np.array_equal(np.array(g[k]), w[k]), (tag, part, k)
        for k in FLOATS:
            assert np.array(g[k]).dtype == f8 and np.array(g[k]).shape == w[k].shape, (tag, part, k)
            assert np.array_equal(bits(g[k]), bits(w[k])), (tag, part, k, np.array(g[k]).ravel()[:4], w[k].ravel()[:4])
            assert np.array_equal(bits(g['field'][k]), bits(w['field'][k])), (tag, part, 'field', k)
        for k in ('cells', 'skipped'):
            assert np.array_equal(np.array(g['field'][k]), w['field'][k]), (tag, part, 'field', k)
        if 'labels' in w:
            assert np.array_equal(np.array(g['labels']), w['labels']), (tag, part, 'labels')
    assert got['grid'] == want['grid']


def summed(res, ospec, observed, domain, tag):
    """The sums of `res` against the rule applied to the maps `res` itself carries; then SAL of the result."""
    spec = ospec.fractions
    plane = maps_of(res)['values'][spec.field][spec.plane]
    want = OB().cells(ospec, plane, observed, domain)
    assert (want['volume'] != 0).any() and (want['observed']['volume'] != 0).any(), (tag, 'the rule finds no object with a volume')
    assert want['field']['cells'].all() and want['observed']['field']['cells'] > 0, (tag, 'the rule sums no cell')
    got = res['composite']['objects']
    same_sums(got, want, tag)
    for t in range(len(spec.thresholds)):
        a, b = OB().sal(got, threshold=t), OB().sal(want, threshold=t)
        for k in ('S', 'A', 'L', 'L1', 'L2'):
            assert a[k].shape == (want['n_objects'].shape[0],) and np.array_equal(bits(a[k]), bits(b[k])), (tag, 'sal', t, k)
    first = OB().sal(got, threshold=0)
    assert np.isfinite(first['A']).all() and np.isfinite(first['L1']).all(), (tag, first)
    c = OB().weighted_centroids(got)
    assert c.shape == want['volume'].shape + (2,) and np.isfinite(c[want['volume'] != 0]).all()
    return want


def test_single_sweep_page_locked_and_device_outputs():
    import torch
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = OB().Objects(spec, connectivity=8, max_objects=64, sums=True)
    res = op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain)
    want = summed(res, ospec, observed, domain, 'page-locked')
    assert want['volume'].shape == (1, 4, 64) and np.isfinite(OB().sal(res['composite']['objects'])['S']).all()
    # without the sums: no new key, the same cells
    plain = op.simulate_rays_composite_fss(az, el, OB().Objects(spec, connectivity=8, max_objects=64), observed, domain=domain)['composite']['objects']
    assert not (NEW | {'weight', 'grid'}) & (set(plain) | set(plain['observed']))
    for k in INTS[:-1] + ('labels',):
        assert np.array_equal(np.array(plain[k]), want[k]), k
    # under a weight table (rain rate instead of linear Z), no labels, a block per ray, NULL domain
    tab = OB().Objects(spec, connectivity=4, max_objects=16, labels=False, sums=True, weight=OB().zr_table(db_min=-20.0))
    per_ray = op.simulate_rays_composite_fss(az, el, tab, observed, rays_per_block=1)
    wr = OB().cells(tab, maps_of(per_ray)['values'][spec.field][spec.plane], observed, None)
    assert wr['volume'].shape == (len(az), 4, 16) and (wr['volume'] != 0).any() and (wr['observed']['volume'] != 0).any()
    same_sums(per_ray['composite']['objects'], wr, 'table, a block per ray')
    assert per_ray['composite']['objects']['weight'] is tab.weight
    # device-resident outputs: everything is a device pointer
    nt = len(spec.thresholds)
    dv = {k: torch.full((1, len(cspec.planes(k)), cspec.n_y, cspec.n_x), 77.0, dtype=torch.float32, device='cuda') for k in cspec.fields}
    dev = {'count': torch.full((1, len(cspec.fields), cspec.n_y, cspec.n_x), 77, dtype=torch.int64, device='cuda'),
           'sums': torch.full((1, nt, len(spec.radii), 3), 77, dtype=torch.int64, device='cuda'),
           'totals': torch.full((1, nt, 3), 77, dtype=torch.int64, device='cuda'),
           'n_objects': torch.full((2, nt), 77, dtype=torch.int32, device='cuda'),
           'table': torch.full((2, nt, ospec.max_objects, 10), 77, dtype=torch.int32, device='cuda'),
           'labels': torch.full((2, nt, cspec.n_y, cspec.n_x), 77, dtype=torch.int32, device='cuda'),
           'volume': torch.full((2, nt, ospec.max_objects, 3), 77.0, dtype=torch.float64, device='cuda'),
           'skipped': torch.full((2, nt, ospec.max_objects), 77, dtype=torch.int32, device='cuda'),
           'field': torch.full((2, 3), 77.0, dtype=torch.float64, device='cuda'),
           'field_cells': torch.full((2, 2), 77, dtype=torch.int32, device='cuda'),
           'observed': torch.from_numpy(observed).cuda(), 'domain': torch.from_numpy(domain).cuda()}
    entry = dict({k: a.data_ptr() for k, a in dev.items()}, values={k: a.data_ptr() for k, a in dv.items()})
    op.simulate_rays_composite_fss(az, el, ospec, None, phase=1, device_outputs={'composite': entry})
    op.wait()
    assert (dev['volume'] == 77).all().item() and (dev['field_cells'] == 77).all().item()       # (nothing before the pass finishes)
    op.simulate_rays_composite_fss(az, el, ospec, None, phase=2, device_outputs={'composite': entry})
    op.wait()
    # (the same sweep folded twice: maxima are those of one, so the plane and its sums are, too)
    assert same(dv['ZH'].cpu().numpy()[:, 0], maps_of(res)['values']['ZH']['max'])
    host = {k: a.cpu().numpy() for k, a in dev.items()}
    got = OB().result(ospec, host['n_objects'].view(u4), host['table'].view(u4), host['labels'],
                      (host['volume'], host['skipped'].view(u4), host['field'], host['field_cells'].view(u4)))
    same_sums(got, want, 'device')


def test_ensemble_a_block_per_member_and_chunks_joined():
    op, _, _ = E.ensemble_operator(NAME)
    _, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = OB().Objects(spec, connectivity=8, max_objects=64, sums=True)
    got = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain)
    want = summed(got, ospec, observed, domain, 'ensemble')
    assert want['volume'].shape == (3, 4, 64) and want['field']['volume'].shape == (3,)
    assert not np.array_equal(bits(want['volume'][0]), bits(want['volume'][1]))
    op.sequence_memory_budget = 1
    cut = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain)
    op.sequence_memory_budget = None
    same_sums(cut['composite']['objects'], want, 'ensemble in chunks')
    assert np.array(cut['composite']['objects']['field']['cells']).shape == (3,)
    op.close()
