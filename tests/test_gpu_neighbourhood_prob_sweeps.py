"""Neighbourhood ensemble probabilities on the GPU through the sweeps (a cpol_fractions_ensemble on a scored finishing call):
res['composite']['probabilities'] of a call against neighbourhood.ensemble_sums of the per-block maps THE SAME CALL returns,
np.array_equal on integers, and its 'fractions' against the call with the Fractions alone.  The setup is the FSS sweep tests':
the golden radial c2_rsg, seven rays, a 17 x 23 grid, the observed map the composite of the case's second cube, thresholds that
are values of the forecast map; the rule's own sums are asserted non-zero, so no test passes on an idle kernel."""
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_composite_sweeps import assert_maps, maps_of, same
from test_gpu_histogram_sweeps import _ops
import test_gpu_neighbourhood_sweeps as NS
from test_gpu_neighbourhood_sweeps import KEYS, RADII, assert_scores, captured

pytestmark = pytest.mark.gpu

NAME = 'c2_rsg'
f4, u1, u4, u8 = np.float32, np.uint8, np.uint32, np.uint64
SUMS = ('diff2', 'forecast2', 'observed2')
MAPS = ('member_sum', 'member_any')


def NB():
    from cosmo_pol_amd import neighbourhood
    return neighbourhood


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


def assert_prob(got, want, pspec, tag):
    for k in SUMS + ('reliability',):
        assert got[k].dtype == u8 and np.array_equal(np.array(got[k]), want[k]), (tag, k, np.array(got[k]).ravel()[:8], want[k].ravel()[:8])
    for k, on in zip(MAPS, (pspec.maps, pspec.any_maps)):
        assert (k in got) == on, (tag, k)
        if on:
            assert got[k].dtype == u4 and np.array_equal(np.array(got[k]), want[k]), (tag, k)
    assert got['n_blocks'] == want['n_blocks'] and np.array_equal(got['radii'], want['radii']), tag
    assert np.array_equal(got['thresholds'], want['thresholds']), tag
    assert want['forecast2'].any() and want['observed2'].any() and want['diff2'].any(), (tag, 'the rule counts nothing')
    assert (want['reliability'].sum(axis=(-2, -1)) > 0).all(), tag


def probed(res, pspec, observed, domain, tag):
    """'probabilities' of `res` against the rule applied to the maps `res` itself carries; 'fractions' against its rule too."""
    maps = maps_of(res)
    plane = maps['values'][pspec.fractions.field]['max']
    want = NB().ensemble_sums(pspec, plane, observed, domain)
    assert want['n_blocks'] == plane.shape[0]
    assert_prob(res['composite']['probabilities'], want, pspec, tag)
    assert_scores(res['composite']['fractions'], NB().sums(pspec.fractions, plane, observed, domain), tag)
    return maps, want


def test_ensemble():
    """A block per member: NEP, NMEP, the ensemble FSS's sums and the reliability table of the three members; one block of all
    members' gates with per_member=False; a member list in chunks is refused."""
    op, _, _ = E.ensemble_operator(NAME)
    _, az, el, cspec, spec, observed, domain = setup(NAME)
    pspec = NB().Probabilities(spec, maps=True, any_maps=True)
    got = op.simulate_rays_ensemble_composite_fss(az, el, pspec, observed, domain=domain)
    maps, want = probed(got, pspec, observed, domain, 'ensemble')
    assert want['reliability'].shape == (4, len(RADII), 4, 2) and want['member_any'].max() == 3
    print('cells by the number of members that exceed, radius 0:', want['reliability'][:, 0].sum(axis=-1).tolist())
    plain = op.simulate_rays_ensemble_composite_fss(az, el, spec, observed, domain=domain)
    assert 'probabilities' not in plain['composite']
    assert_maps(maps_of(plain), maps, cspec, 'the Fractions alone')
    for k in KEYS:
        assert np.array_equal(np.array(plain['composite']['fractions'][k]), np.array(got['composite']['fractions'][k])), k
    # the host helpers on the device's result
    pr = got['composite']['probabilities']
    efss = NB().fss(pr)
    assert efss.shape == (4, len(RADII)) and ((efss > 0.0) & (efss < 1.0)).any()
    nep = NB().nep(pr, NB().window_cells(pspec, domain))
    assert np.nanmax(nep) <= 1.0 and np.nanmax(NB().nmep(pr)) == 1.0 and (NB().brier(pr) >= 0.0).all()
    # without a domain and without the maps
    bare = NB().Probabilities(spec)
    probed(op.simulate_rays_ensemble_composite_fss(az, el, bare, observed), bare, observed, None, 'ensemble, no domain, no maps')
    # one block of all members' gates
    whole = op.simulate_rays_ensemble_composite_fss(az, el, pspec, observed, domain=domain, per_member=False)
    _, ww = probed(whole, pspec, observed, domain, 'ensemble, one map')
    assert ww['n_blocks'] == 1 and ww['reliability'].shape == (4, len(RADII), 2, 2)
    for k in SUMS:                                    # (M == 1: block 0's row of `sums`)
        assert np.array_equal(ww[k], np.array(whole['composite']['fractions'][k])[0]), k
    # a member list cut into chunks
    op.sequence_memory_budget = 1
    try:
        for per_member in (True, False):
            with pytest.raises(ValueError, match='needs the members in one chunk'):
                op.simulate_rays_ensemble_composite_fss(az, el, pspec, observed, domain=domain, per_member=per_member)
    finally:
        op.sequence_memory_budget = None
    probed(op.simulate_rays_ensemble_composite_fss(az, el, pspec, observed, domain=domain), pspec, observed, domain, 'after the refusal')
    op.close()


def test_ensemble_device_outputs():
    import torch
    op, _, _ = E.ensemble_operator(NAME)
    _, az, el, cspec, spec, observed, domain = setup(NAME)
    pspec = NB().Probabilities(spec, maps=True)
    host = op.simulate_rays_ensemble_composite_fss(az, el, pspec, observed, domain=domain)
    maps, want = probed(host, pspec, observed, domain, 'host outputs')
    nt, nr, M = len(spec.thresholds), len(RADII), 3

    def filled(shape, dtype=torch.int64):
        return torch.full(shape, 77, dtype=dtype, device='cuda')
    dv = {k: torch.full((M, len(cspec.planes(k)), cspec.n_y, cspec.n_x), 77.0, dtype=torch.float32, device='cuda') for k in cspec.fields}
    dc, ds, dt = filled((M, len(cspec.fields), cspec.n_y, cspec.n_x)), filled((M, nt, nr, 3)), filled((M, nt, 3))
    dp, dr, dm = filled((nt, nr, 3)), filled((nt, nr, M + 1, 2)), filled((nt, nr, cspec.n_y, cspec.n_x), torch.int32)
    d_obs, d_dom = torch.from_numpy(observed).cuda(), torch.from_numpy(domain).cuda()
    entry = {'values': {k: a.data_ptr() for k, a in dv.items()}, 'count': dc.data_ptr(), 'observed': d_obs.data_ptr(),
             'domain': d_dom.data_ptr(), 'sums': ds.data_ptr(), 'totals': dt.data_ptr(), 'prob_sums': dp.data_ptr(),
             'reliability': dr.data_ptr(), 'member_sum': dm.data_ptr()}
    op.simulate_rays_ensemble_composite_fss(az, el, pspec, None, device_outputs={'composite': entry})
    op.wait()
    assert same(dv['ZH'].cpu().numpy()[:, 0], maps['values']['ZH']['max'])
    got = NB().ensemble_result(spec, M, dp.cpu().numpy().view(u8), dr.cpu().numpy().view(u8), dm.cpu().numpy().view(u4))
    assert_prob(got, want, pspec, 'device outputs')
    assert_scores(NB().result(spec, ds.cpu().numpy().view(u8), dt.cpu().numpy().view(u8)),
                  NB().sums(spec, maps['values']['ZH']['max'], observed, domain), 'device outputs')
    with pytest.raises(ValueError, match="unknown entry 'member_any'"):          # (a map that was not asked for)
        op.simulate_rays_ensemble_composite_fss(az, el, pspec, None, device_outputs={'composite': dict(entry, member_any=dm.data_ptr())})
    op.close()


def test_blocks_of_rays_and_a_pass_cut_by_phase():
    """simulate_rays_composite_fss: a block per ray; and a pass of three calls, scored once, at its finish."""
    op, az, el, cspec, spec, observed, domain = setup(NAME)
    pspec = NB().Probabilities(spec, any_maps=True)
    per_ray = op.simulate_rays_composite_fss(az, el, pspec, observed, domain=domain, rays_per_block=1)
    _, want = probed(per_ray, pspec, observed, domain, 'a block per ray')
    assert want['n_blocks'] == len(az) and want['reliability'].shape[2] == len(az) + 1
    whole = op.simulate_rays_composite_fss(az, el, pspec, observed, domain=domain)
    good, one = probed(whole, pspec, observed, domain, 'one call')
    parts = []
    for rows, phase in ((slice(0, 3), 1), (slice(3, 5), 0), (slice(5, 7), 2)):
        res, seen = captured(op, lambda: op.simulate_rays_composite_fss(az[rows], el[rows], pspec, observed, domain=domain, phase=phase))
        assert seen['slots'] == (True, phase == 2)                # (the structs go with the finishing call alone)
        parts.append(res)
    assert 'composite' not in parts[0] and 'composite' not in parts[1]
    assert_maps(maps_of(parts[2]), good, cspec, 'three calls')
    assert_prob(parts[2]['composite']['probabilities'], one, pspec, 'three calls')
    assert_scores(parts[2]['composite']['fractions'], NB().sums(spec, good['values']['ZH']['max'], observed, domain), 'three calls')


def test_network():
    from test_gpu_composite_network import network, rule
    op, az, elevations, radars, gates, cspec = network.__wrapped__(NAME)       # (not the cached one: its operator is closed)
    forecast = rule(cspec, NAME, [(gates[r][e], r) for r in range(2) for e in range(2)])['values']['ZH']['max'][0]
    observed = np.roll(forecast, 1, axis=1)
    v = np.sort(forecast[np.isfinite(forecast)].astype(np.float64))
    fr = NB().Fractions(cspec, 'ZH', [float(v[int(q * (v.size - 1))]) for q in (0.25, 0.5, 0.75)], [0, 2])
    pspec = NB().Probabilities(fr, maps=True, any_maps=True)
    res = op.get_network_composite_fss(radars, elevations, pspec, observed, azimuths=az)
    assert same(maps_of(res)['values']['ZH']['max'][0], forecast)
    probed(res, pspec, observed, None, 'network')
    assert all('composite' not in sw for per in res['sweeps'] for sw in per)          # reduced once, at the end of the pass
    plain = op.get_network_composite_fss(radars, elevations, fr, observed, azimuths=az)
    assert 'probabilities' not in plain['composite']
    for k in KEYS:
        assert np.array_equal(np.array(plain['composite']['fractions'][k]), np.array(res['composite']['fractions'][k])), k
    op.close()


def test_a_call_without_probabilities_is_left_alone():
    """Sweeps of one geometry with the Fractions alone, before and behind calls with a Probabilities: the same maps and scores bit
    for bit, the same stencil forms and launch forms sweep by sweep; the cpol_fractions of such a call carries no flag."""
    from test_gpu_ensemble import case, load, operator
    from test_gpu_histogram_sweeps import arrays
    from test_gpu_composite_sweeps import same_gates
    from cosmo_pol_amd import _native as N
    conf, luts, cubes, _, _ = case(NAME)
    _, az, el, cspec, spec, observed, domain = setup(NAME)
    pspec = NB().Probabilities(spec, maps=True, any_maps=True)
    seen = {}
    for with_prob in (False, True):
        op = operator(conf, luts)
        load(op, cubes[0])
        st, forms, out = [], [], []
        for i in range(5):
            res = op.simulate_rays_composite_fss(az, el, pspec if with_prob else spec, observed, domain=domain, keep_gates=True)
            out.append((arrays(res), maps_of(res), res['composite']['fractions']))
            assert ('probabilities' in res['composite']) == with_prob
            st.append(op.stencil_state()['form'])
            forms.append(op._ctx.launch_forms())
        if with_prob:                         # ... and a Fractions call behind them returns what it returned before
            ctx, slots = op._ctx, []
            orig = ctx.run_sweep

            def spy(p, t, o):
                slots.append(bool(o.fractions.contents.n_radii & N.FRAC_ENSEMBLE))
                return orig(p, t, o)
            ctx.run_sweep = spy
            try:
                after = op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain, keep_gates=True)
                op.simulate_rays_composite_fss(az, el, pspec, observed, domain=domain)
            finally:
                del ctx.run_sweep
            assert slots == [False, True] and 'probabilities' not in after['composite']
            assert_maps(maps_of(after), seen[False][2][0][1], cspec, 'a Fractions call behind calls with a Probabilities')
            for k in KEYS:
                assert np.array_equal(np.array(after['composite']['fractions'][k]), np.array(seen[False][2][0][2][k])), k
        seen[with_prob] = (st, forms, out)
        op.close()
    print('stencil forms without / with the probabilities:', seen[False][0], seen[True][0])
    assert seen[False][0] == seen[True][0] and seen[True][0][-1] == 2
    assert seen[False][1] == seen[True][1]
    for i in range(5):
        for k, v in seen[False][2][i][0].items():
            assert same_gates(seen[True][2][i][0][k], v), (i, k)
        assert_maps(seen[True][2][i][1], seen[False][2][i][1], cspec, 'sweep %d' % i)
        for k in KEYS:
            assert np.array_equal(np.array(seen[True][2][i][2][k]), np.array(seen[False][2][i][2][k])), (i, k)
