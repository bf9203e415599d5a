"""The match of the object cells on the GPU through the sweeps (a cpol_objects_match on a scored finishing call): the pieces and
`covered` of a call against objects.cells of the maps THE SAME CALL returns, np.array_equal; `pairs`, `match` and `contingency`
on the result.  The small operator case of tests/test_gpu_objects_sweeps.py: the observed map is the composite of the case's
second cube, the thresholds are values of the forecast map itself.  The rule is asserted to find pieces, so no test passes on
empty maps or on an idle kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_composite_sweeps import assert_maps, maps_of, same
from test_gpu_histogram_sweeps import _ops
import test_gpu_neighbourhood_sweeps as NS
from test_gpu_neighbourhood_sweeps import KEYS as SUMS, captured

pytestmark = pytest.mark.gpu

f4, u1, u4, u8, i4, i8 = np.float32, np.uint8, np.uint32, np.uint64, np.int32, np.int64
CELLS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')
PIECES = ('n_pieces', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'forecast', 'observed')
NEW = {'pieces', 'covered', 'covered_observed'}
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


def match_spec(spec, **kw):
    kw.setdefault('connectivity', 8)
    kw.setdefault('max_objects', 64)
    kw.setdefault('max_pieces', 128)
    return OB().Objects(spec, match=True, **kw)


def same_all(got, want, tag):
    for part, g, w in (('blocks', got, want), ('observed', got['observed'], want['observed'])):
        for k in CELLS:
            assert np.array(g[k]).dtype == u4 and np.array_equal(np.array(g[k]), w[k]), (tag, part, k)
        assert np.array_equal(np.array(g['peak']).view(u4), w['peak'].view(u4)), (tag, part, 'peak')
        assert ('labels' in g) == ('labels' in w), (tag, part)
        if 'labels' in w:
            assert np.array_equal(np.array(g['labels']), w['labels']), (tag, part, 'labels')
    assert sorted(got['pieces']) == sorted(PIECES), tag
    for k in PIECES:
        g = np.array(got['pieces'][k])
        assert g.dtype == u4 and g.shape == want['pieces'][k].shape and np.array_equal(g, want['pieces'][k]), (tag, 'pieces', k, g.ravel()[:8])
    for k in ('covered', 'covered_observed'):
        g = np.array(got[k])
        assert g.dtype == u4 and g.shape == want[k].shape and np.array_equal(g, want[k]), (tag, k, g.ravel()[:8], want[k].ravel()[:8])


def matched(res, ospec, observed, domain, tag):
    """The cells and the match of `res` against the rule applied to the maps `res` itself carries; then the host folds: `pairs` and
    `contingency` are consistent with `covered`."""
    spec = ospec.fractions
    plane = maps_of(res)['values'][spec.field][spec.plane]
    want = OB().cells(ospec, plane, observed, domain)
    assert want['pieces']['n_pieces'].any() and want['n_objects'].any() and want['observed']['n_objects'].any(), (tag, 'the rule finds no piece')
    got = res['composite']['objects']
    same_all(got, want, tag)
    n_blocks, n_thr = want['n_objects'].shape
    for t in range(n_thr):
        con = OB().contingency(got, t)
        cov, cov_o = np.array(got['covered'])[:, t], np.array(got['covered_observed'])[:, t]
        n_f, n_o = want['n_objects'][:, t].astype(i8), int(want['observed']['n_objects'][t])
        fits = (n_f <= ospec.max_objects) & (n_o <= ospec.max_objects)
        assert np.array_equal(con['hits'][fits], (cov_o > 0).sum(axis=-1)[fits]), (tag, t, 'hits')
        assert np.array_equal((con['hits'] + con['misses'])[fits], np.full(n_blocks, n_o)[fits]), (tag, t, 'hits and misses')
        assert np.array_equal(con['false_alarms'][fits], (n_f - (cov > 0).sum(axis=-1))[fits]), (tag, t, 'false alarms')
        assert (con['hits'][~fits] == -1).all() and np.isnan(con['csi'][~fits]).all(), (tag, t)
        for b in range(n_blocks):
            if int(want['pieces']['n_pieces'][b, t]) > ospec.max_pieces:
                with pytest.raises(ValueError, match='a partial fold is not returned'):
                    OB().pairs(got, b, t)
                continue
            p = OB().pairs(got, b, t)
            # the pairs' areas summed per object are `covered`, for the objects with a row
            for side, c in (('forecast', cov[b]), ('observed', cov_o[b])):
                rows = p[side] <= ospec.max_objects
                assert np.array_equal(np.bincount(p[side][rows] - 1, weights=p['area'][rows], minlength=ospec.max_objects).astype(i8), c.astype(i8)), (tag, b, t, side)
            assert int(p['pieces'].sum()) == int(want['pieces']['n_pieces'][b, t])
        m = OB().match(got, t)
        ok = want['pieces']['n_pieces'][:, t] <= ospec.max_pieces
        assert np.array_equal((m['partner'][ok] > 0), cov[ok] > 0) and (m['area'][ok] <= cov[ok]).all(), (tag, t, 'match')
        assert (m['partner'][~ok] == -1).all(), (tag, t)
    return want


def test_single_sweep_blocks_of_rays_and_terms():
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    for kw in ({'connectivity': 4}, {'connectivity': 8}, {'connectivity': 8, 'min_area': 3}, {'connectivity': 4, 'max_objects': 2},
               {'connectivity': 4, 'max_pieces': 1}, {'connectivity': 8, 'labels': False}):
        ospec = match_spec(spec, **kw)
        res = op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain)
        want = matched(res, ospec, observed, domain, (NAME, sorted(kw.items())))
        assert want['pieces']['n_pieces'].shape == (1, 4) and want['covered'].shape == (1, 4, ospec.max_objects)
    ospec = match_spec(spec)
    per_ray = op.simulate_rays_composite_fss(az, el, ospec, observed, rays_per_block=1)          # (NULL domain: every cell)
    want = matched(per_ray, ospec, observed, None, 'a block per ray')
    assert want['pieces']['n_pieces'].shape == (len(az), 4) and want['pieces']['bbox'].shape == (len(az), 4, 128, 4)
    assert want['covered_observed'].shape == (len(az), 4, 64) and not np.array_equal(want['covered'][0], want['covered'][-1])
    # without the match: no new key, the same cells and scores
    plain = op.simulate_rays_composite_fss(az, el, OB().Objects(spec, connectivity=8, max_objects=64), observed, rays_per_block=1)
    assert not NEW & set(plain['composite']['objects'])
    for k in CELLS + ('labels',):
        assert np.array_equal(np.array(plain['composite']['objects'][k]), want[k]), k
    for k in SUMS:
        assert np.array_equal(np.array(plain['composite']['fractions'][k]), np.array(per_ray['composite']['fractions'][k])), k
    # the exact sums beside the match
    both = OB().Objects(spec, connectivity=8, max_objects=64, sums=True, match=True)
    res = op.simulate_rays_composite_fss(az, el, both, observed, domain=domain)
    want = matched(res, both, observed, domain, 'sums and match')
    for k in ('volume', 'moment_x', 'moment_y'):
        assert np.array_equal(np.array(res['composite']['objects'][k]).view(u8), want[k].view(u8)), k


def direct(op, ospec, az, p, t, observed, domain, change=None):
    """One blocking cpol_run_sweep (outputs_on_device 0) with plain host arrays -> (maps, the objects' result)."""
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import composite as CP
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
    om = okeep[0]
    n, table = np.full((2, nt), 77, u4), np.full((2, nt, ospec.max_objects, 10), 77, u4)
    labels = np.full((2, nt, cspec.n_y, cspec.n_x), 77, i4)
    o.n_objects, o.table, o.labels = n.ctypes.data, table.ctypes.data, labels.ctypes.data
    match = [np.full((1, nt), 77, u4), np.full((1, nt, ospec.max_pieces, 10), 77, u4), np.full((1, nt, 2, ospec.max_objects), 77, u4)]
    om.n_pieces, om.pieces, om.covered = [q.ctypes.data for q in match]
    if change:
        change(om)
    out = N.Outputs()
    out.composite, out.fractions = C.pointer(c), C.pointer(f)
    q = N.SweepParams.from_buffer_copy(p)
    q.outputs_on_device = 0
    op._ctx.run_sweep(q, t, out)
    op.wait()
    del keep, okeep
    maps = {'values': {k: {p_: vals[k][:, j] for j, p_ in enumerate(cspec.planes(k))} for k in cspec.fields},
            'count': {k: cnt[:, i] for i, k in enumerate(cspec.fields)}}
    return maps, OB().result(ospec, n, table, labels, None, match)


def test_output_modes_and_refusals():
    """Page-locked buffers (waited for, and pinned=True + wait), blocking host buffers and device pointers carry the same match;
    every refusal of the library is followed by a good call."""
    import torch
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = match_spec(spec)
    locked, seen = captured(op, lambda: op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain))
    want = matched(locked, ospec, observed, domain, 'page-locked')
    good = maps_of(locked)
    lazy = op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain, pinned=True)
    op.wait()
    same_all(lazy['composite']['objects'], want, 'pinned')
    maps, got = direct(op, ospec, az, seen['p'], seen['t'], observed, domain)
    assert_maps(maps, good, cspec, 'blocking')
    same_all(got, want, 'blocking')
    for word, change in (('pad_ .* must lie in 0 ... 65535', lambda om: setattr(om.o, 'pad_', -1)),
                         ('pad_ .* must lie in 0 ... 65535', lambda om: setattr(om.o, 'pad_', 65536)),
                         ('n_pieces, pieces or covered is NULL', lambda om: setattr(om, 'n_pieces', None)),
                         ('n_pieces, pieces or covered is NULL', lambda om: setattr(om, 'pieces', None)),
                         ('n_pieces, pieces or covered is NULL', lambda om: setattr(om, 'covered', None))):
        with pytest.raises(ValueError, match='cpol_objects: ' + word):
            direct(op, ospec, az, seen['p'], seen['t'], observed, domain, change=change)
        same_all(direct(op, ospec, az, seen['p'], seen['t'], observed, domain)[1], want, ('after the refusal', word))
    # a zero pad_: the match is off, its three arrays untouched, the cells as ever
    _, got = direct(op, ospec, az, seen['p'], seen['t'], observed, domain, change=lambda om: setattr(om.o, 'pad_', 0))
    assert (got['pieces']['n_pieces'] == 77).all() and (got['pieces']['area'] == 77).all() and (got['covered'] == 77).all()
    assert np.array_equal(got['area'], want['area']) and np.array_equal(got['labels'], want['labels'])
    # device outputs: everything is a device pointer; a pass of two calls writes nothing before its finish
    nt = len(spec.thresholds)
    dv = {k: torch.full((1, len(cspec.planes(k)), cspec.n_y, cspec.n_x), 77.0, dtype=torch.float32, device='cuda') for k in cspec.fields}
    dev = {'count': torch.full((1, len(cspec.fields), cspec.n_y, cspec.n_x), 77, dtype=torch.int64, device='cuda'),
           'sums': torch.full((1, nt, len(spec.radii), 3), 77, dtype=torch.int64, device='cuda'),
           'totals': torch.full((1, nt, 3), 77, dtype=torch.int64, device='cuda'),
           'n_objects': torch.full((2, nt), 77, dtype=torch.int32, device='cuda'),
           'table': torch.full((2, nt, ospec.max_objects, 10), 77, dtype=torch.int32, device='cuda'),
           'labels': torch.full((2, nt, cspec.n_y, cspec.n_x), 77, dtype=torch.int32, device='cuda'),
           'n_pieces': torch.full((1, nt), 77, dtype=torch.int32, device='cuda'),
           'pieces': torch.full((1, nt, ospec.max_pieces, 10), 77, dtype=torch.int32, device='cuda'),
           'covered': torch.full((1, nt, 2, ospec.max_objects), 77, dtype=torch.int32, device='cuda'),
           'observed': torch.from_numpy(observed).cuda(), 'domain': torch.from_numpy(domain).cuda()}
    entry = dict({k: a.data_ptr() for k, a in dev.items()}, values={k: a.data_ptr() for k, a in dv.items()})
    op.simulate_rays_composite_fss(az, el, ospec, None, phase=1, device_outputs={'composite': entry})
    op.wait()
    assert (dev['n_pieces'] == 77).all().item() and (dev['pieces'] == 77).all().item() and (dev['covered'] == 77).all().item()
    op.simulate_rays_composite_fss(az, el, ospec, None, phase=2, device_outputs={'composite': entry})
    op.wait()
    # (the same sweep folded twice: maxima and minima are those of one, so the plane, its cells and their match are, too)
    assert same(dv['ZH'].cpu().numpy()[:, 0], good['values']['ZH']['max'])
    host = {k: a.cpu().numpy() for k, a in dev.items()}
    got = OB().result(ospec, host['n_objects'].view(u4), host['table'].view(u4), host['labels'], None,
                      [host['n_pieces'].view(u4), host['pieces'].view(u4), host['covered'].view(u4)])
    same_all(got, want, 'device')
    matched(op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain), ospec, observed, domain, 'after the device call')


def test_ensemble_a_block_per_member_in_one_chunk_and_one_chunk_per_member():
    op, _, _ = E.ensemble_operator(NAME)
    _, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = match_spec(spec)
    got = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain)
    want = matched(got, ospec, observed, domain, 'ensemble')
    assert want['pieces']['n_pieces'].shape == (3, 4) and want['covered'].shape == (3, 4, 64)
    assert not np.array_equal(want['pieces']['area'][0], want['pieces']['area'][1])
    op.select_member(1)
    alone = op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain)['composite']['objects']
    for k in PIECES:
        assert np.array_equal(np.array(alone['pieces'][k]), want['pieces'][k][1:2]), k
    assert np.array_equal(np.array(alone['covered_observed']), want['covered_observed'][1:2])
    op.select_member(0)
    op.sequence_memory_budget = 1
    cut = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain)
    cut_whole = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain, per_member=False)
    op.sequence_memory_budget = None
    same_all(cut['composite']['objects'], want, 'ensemble in chunks')
    matched(cut, ospec, observed, domain, 'ensemble in chunks, folds')
    whole = op.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain, per_member=False)
    ww = matched(whole, ospec, observed, domain, 'ensemble, one map')
    assert ww['pieces']['n_pieces'].shape == (1, 4)
    same_all(cut_whole['composite']['objects'], ww, 'ensemble in chunks, one map')
    op.close()
