"""The track of the object cells on the GPU through the sweeps (a cpol_objects_track on a scored finishing call): the correlation,
the shift, the pieces and `covered` of a call against objects.cells of the planes THE SAME CALL returns, np.array_equal; `links`,
`tracks` and `motion` on the device result.  The small operator case of tests/test_gpu_objects_sweeps.py; the blocks are the
case's rays scanned again at rising elevations, or the scan times of a short series.  The rule is asserted to find pieces, so no
test passes on empty maps or on an idle kernel."""
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_composite_sweeps import maps_of
from test_gpu_histogram_sweeps import _ops
import test_gpu_neighbourhood_sweeps as NS

pytestmark = pytest.mark.gpu

f4, u1, u4, u8, i4, i8 = np.float32, np.uint8, np.uint32, np.uint64, np.int32, np.int64
CELLS = ('n_objects', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak_cell')
PIECES = ('n_pieces', 'first', 'area', 'sum_x', 'sum_y', 'bbox', 'forecast', 'observed')
TRACK = ('correlation', 'shift', 'n_pieces', 'pieces', 'covered')
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


def track_spec(spec, **kw):
    kw.setdefault('connectivity', 8)
    kw.setdefault('max_objects', 64)
    kw.setdefault('max_track_pieces', 128)
    if 'shifts' not in kw:
        kw.setdefault('max_shift', 4)
    return OB().Objects(spec, track=True, **kw)


def blocks_of(az, el, n_blocks, step=0.5):
    """The case's rays `n_blocks` times over, block b at the elevations el + b * step: (azimuths, elevations, rays per block)."""
    return np.tile(az, n_blocks), np.concatenate([np.asarray(el, dtype=np.float64) + b * step for b in range(n_blocks)]), len(az)


def same_all(got, want, tag):
    for part, g, w in (('blocks', got, want), ('observed', got['observed'], want['observed'])):
        for k in CELLS:
            assert np.array(g[k]).dtype == u4 and np.array_equal(np.array(g[k]), w[k]), (tag, part, k)
        assert np.array_equal(np.array(g['peak']).view(u4), w['peak'].view(u4)), (tag, part, 'peak')
        if 'labels' in w:
            assert np.array_equal(np.array(g['labels']), w['labels']), (tag, part, 'labels')
    assert ('pieces' in got) == ('pieces' in want), tag
    if 'pieces' in want:
        for k in PIECES:
            assert np.array_equal(np.array(got['pieces'][k]), want['pieces'][k]), (tag, 'pieces', k)
        assert np.array_equal(np.array(got['covered']), want['covered']) and np.array_equal(np.array(got['covered_observed']), want['covered_observed']), tag
    assert sorted(got['track']) == sorted(TRACK), tag
    for k in TRACK:
        w = want['track'][k]
        if w is None:
            assert got['track'][k] is None, (tag, k)
            continue
        g = np.array(got['track'][k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (tag, 'track', k, g.ravel()[:12], w.ravel()[:12])


def tracked(res, ospec, observed, domain, tag):
    """The cells and the track of `res` against the rule applied to the planes `res` itself carries; then the host folds run on
    the device result and agree with `covered`."""
    spec = ospec.fractions
    plane = maps_of(res)['values'][spec.field][spec.plane]
    want = OB().cells(ospec, plane, observed, domain)
    assert want['track']['n_pieces'].any() and want['n_objects'].any(), (tag, 'the rule finds no piece')
    got = res['composite']['objects']
    same_all(got, want, tag)
    P, n_thr = want['track']['n_pieces'].shape
    for t in range(n_thr):
        if int(want['track']['n_pieces'][:, t].max()) > ospec.max_track_pieces:
            with pytest.raises(ValueError, match='a partial fold is not returned'):
                OB().tracks(got, t)
            continue
        for p in range(P):
            L = OB().links(got, p, t)
            for side, who in ((0, 'earlier'), (1, 'later')):
                rows = L[who] <= ospec.max_objects
                assert np.array_equal(np.bincount(L[who][rows] - 1, weights=L['area'][rows], minlength=ospec.max_objects).astype(i8),
                                      np.array(got['track']['covered'])[p, t, side].astype(i8)), (tag, p, t, who)
        tk = OB().tracks(got, t)
        n = want['n_objects'][:, t].astype(i8)
        assert [a.size for a in tk['track_id']] == n.tolist() and all((a > 0).all() for a in tk['track_id']), (tag, t)
        n_tracks = tk['birth'].size
        assert n_tracks == int(n[0]) + sum(int(n[p + 1]) - len(tk['inherited'][p]) for p in range(P)), (tag, t, 'every object inherits or opens a track')
        assert (tk['death'] >= tk['birth']).all() and (tk['parent'] <= n_tracks).all() and (tk['merged_into'] <= n_tracks).all()
        m = OB().motion(got, t)
        assert np.array_equal(m['shift'], want['track']['shift'][:, t]) and len(m['links']) == P
        assert all(np.array_equal(m['links'][p]['earlier'], tk['inherited'][p][:, 0]) for p in range(P))
    return want


def test_blocks_of_rays_terms_and_what_rides_beside():
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    az3, el3, rpb = blocks_of(az, el, 3)
    for kw in ({'connectivity': 4}, {'connectivity': 8, 'max_shift': 0}, {'connectivity': 8, 'min_area': 3}, {'connectivity': 4, 'max_objects': 2},
               {'connectivity': 4, 'max_track_pieces': 1}, {'labels': False}, {'shifts': [1, -1]}, {'shifts': np.array([[[0, 0]], [[-2, 3]]])},
               {'match': True, 'max_pieces': 32}, {'sums': True}):
        ospec = track_spec(spec, **kw)
        res = op.simulate_rays_composite_fss(az3, el3, ospec, observed, domain=domain, rays_per_block=rpb)
        want = tracked(res, ospec, observed, domain, (NAME, sorted(kw)))
        assert want['track']['n_pieces'].shape == (2, 4) and want['track']['covered'].shape == (2, 4, 2, ospec.max_objects)
        assert (want['track']['correlation'] is None) == ('shifts' in kw)
    # a block per ray, NULL domain: seven blocks, six pairs
    ospec = track_spec(spec, max_shift=8)
    per_ray = op.simulate_rays_composite_fss(az, el, ospec, observed, rays_per_block=1)
    want = tracked(per_ray, ospec, observed, None, 'a block per ray')
    assert want['track']['shift'].shape == (len(az) - 1, 4, 2) and want['track']['correlation'].shape == (len(az) - 1, 4, 17, 17)
    # without the track: no new key, the same cells and scores
    plain = op.simulate_rays_composite_fss(az, el, OB().Objects(spec, connectivity=8, max_objects=64), observed, rays_per_block=1)
    assert 'track' not in plain['composite']['objects']
    for k in CELLS + ('labels',):
        assert np.array_equal(np.array(plain['composite']['objects'][k]), want[k]), k
    for k in NS.KEYS:
        assert np.array_equal(np.array(plain['composite']['fractions'][k]), np.array(per_ray['composite']['fractions'][k])), k


def test_a_short_series_of_scan_times():
    import test_gpu_timed as T
    op, _, _ = T.series_operator(NAME)
    _, az, el, cspec, spec, observed, domain = setup(NAME)
    times = [100.0, 700.0, 1400.0]
    azt, elt, tt = np.tile(az, 3), np.tile(el, 3), np.repeat(times, len(az))
    for kw in ({}, {'shifts': [0, 1], 'connectivity': 4}):
        ospec = track_spec(spec, **kw)
        res = op.simulate_rays_at_composite_fss(azt, elt, tt, ospec, observed, domain=domain, rays_per_block=len(az))
        want = tracked(res, ospec, observed, domain, ('series', sorted(kw)))
        assert want['track']['n_pieces'].shape == (2, 4)
    with pytest.raises(ValueError, match='yields 1 block'):
        op.simulate_rays_at_composite_fss(az, el, 200.0, track_spec(spec), observed, domain=domain)
    tracked(op.simulate_rays_at_composite_fss(azt, elt, tt, ospec, observed, domain=domain, rays_per_block=len(az)), ospec, observed, domain,
            'after the refusal')
    op.close()


def test_a_volume_folded_over_the_calls_of_a_pass():
    """Two elevations of two blocks: in one call (the block's rows side by side) and as a pass of two calls, one elevation each."""
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = track_spec(spec)
    az, el = np.asarray(az, dtype=np.float64), np.asarray(el, dtype=np.float64)
    half = len(az) // 2
    groups = [(az[:half], el[:half]), (az[half:2 * half], el[half:2 * half])]
    one_az = np.concatenate([np.concatenate([a, a]) for a, _ in groups])
    one_el = np.concatenate([np.concatenate([e, e + 1.0]) for _, e in groups])
    whole = op.simulate_rays_composite_fss(one_az, one_el, ospec, observed, domain=domain, rays_per_block=2 * half)
    want = tracked(whole, ospec, observed, domain, 'one call')
    first = op.simulate_rays_composite_fss(np.concatenate([a for a, _ in groups]), np.concatenate([e for _, e in groups]), ospec, observed,
                                           domain=domain, rays_per_block=half, phase=1)
    assert 'composite' not in first
    last = op.simulate_rays_composite_fss(np.concatenate([a for a, _ in groups]), np.concatenate([e + 1.0 for _, e in groups]), ospec, observed,
                                          domain=domain, rays_per_block=half, phase=2)
    same_all(last['composite']['objects'], want, 'two calls')
    tracked(last, ospec, observed, domain, 'two calls, the rule')


def test_device_outputs_carry_the_same_track():
    import torch
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = track_spec(spec)
    az2, el2, rpb = blocks_of(az, el, 2)
    want = tracked(op.simulate_rays_composite_fss(az2, el2, ospec, observed, domain=domain, rays_per_block=rpb), ospec, observed, domain, 'host')
    lazy = op.simulate_rays_composite_fss(az2, el2, ospec, observed, domain=domain, rays_per_block=rpb, pinned=True)
    op.wait()
    same_all(lazy['composite']['objects'], want, 'pinned')
    nt, side = len(spec.thresholds), 2 * ospec.max_shift + 1

    def full(shape, dtype=torch.int32):
        return torch.full(shape, 77, dtype=dtype, device='cuda')
    dv = {k: full((2, len(cspec.planes(k)), cspec.n_y, cspec.n_x), torch.float32) for k in cspec.fields}
    dev = {'count': full((2, len(cspec.fields), cspec.n_y, cspec.n_x), torch.int64), 'sums': full((2, nt, len(spec.radii), 3), torch.int64),
           'totals': full((2, nt, 3), torch.int64), 'n_objects': full((3, nt)), 'table': full((3, nt, ospec.max_objects, 10)),
           'labels': full((3, nt, cspec.n_y, cspec.n_x)), 'track_correlation': full((1, nt, side, side)), 'track_shift': full((1, nt, 2)),
           'track_n_pieces': full((1, nt)), 'track_pieces': full((1, nt, ospec.max_track_pieces, 10)),
           'track_covered': full((1, nt, 2, ospec.max_objects)),
           'observed': torch.from_numpy(observed).cuda(), 'domain': torch.from_numpy(domain).cuda()}
    entry = dict({k: a.data_ptr() for k, a in dev.items()}, values={k: a.data_ptr() for k, a in dv.items()})
    op.simulate_rays_composite_fss(az2, el2, ospec, None, rays_per_block=rpb, device_outputs={'composite': entry})
    op.wait()
    host = {k: a.cpu().numpy() for k, a in dev.items()}
    got = OB().result(ospec, host['n_objects'].view(u4), host['table'].view(u4), host['labels'], None, None,
                      [host['track_correlation'].view(u4), host['track_shift'], host['track_n_pieces'].view(u4), host['track_pieces'].view(u4),
                       host['track_covered'].view(u4)])
    same_all(got, want, 'device')
    tracked(op.simulate_rays_composite_fss(az2, el2, ospec, observed, domain=domain, rays_per_block=rpb), ospec, observed, domain, 'after the device call')


def test_the_ensemble_entry_points_and_one_block_raise():
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    ospec = track_spec(spec)
    with pytest.raises(ValueError, match='yields 1 block'):
        op.simulate_rays_composite_fss(az, el, ospec, observed, domain=domain)
    az2, el2, rpb = blocks_of(az, el, 2)
    with pytest.raises(ValueError, match='does not broadcast'):
        op.simulate_rays_composite_fss(az2, el2, track_spec(spec, shifts=np.zeros((2, 1, 2), i4)), observed, rays_per_block=rpb)
    tracked(op.simulate_rays_composite_fss(az2, el2, ospec, observed, domain=domain, rays_per_block=rpb), ospec, observed, domain, 'after the refusals')
    ens, _, _ = E.ensemble_operator(NAME)
    for per_member in (True, False):
        with pytest.raises(ValueError, match='members, not times'):
            ens.simulate_rays_ensemble_composite_fss(az, el, ospec, observed, domain=domain, per_member=per_member)
    plain = ens.simulate_rays_ensemble_composite_fss(az, el, OB().Objects(spec, connectivity=8, max_objects=64), observed, domain=domain)
    assert 'track' not in plain['composite']['objects'] and np.array(plain['composite']['objects']['n_objects']).shape == (3, 4)
    ens.close()
