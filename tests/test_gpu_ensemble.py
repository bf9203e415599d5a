"""Ensembles on the GPU: members staged beside the model (cpol_stage_member), cpol_select_member, and the shared-geometry sweep
(cpol_run_sweep_members, k_interp_members) -- every member's arrays against simulate_rays of a fresh operator loaded with that
member alone, bit for bit, and member 0 against the golden file / the oracle."""
import copy
import functools
import os
import sys
import types

import numpy as np
import pytest

import _cases
import gen_golden as GG
import test_gpu_seam as S
from cosmo_pol_oracle import beam, scatter

pytestmark = pytest.mark.gpu

FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL', 'DSPECTRUM', 'mask']
GEOM = ['lats', 'lons', 'dist', 'heights']
# member 2: the bad values tests/test_gpu_bad_values.py plants (rings around the radar, in grid cells), in U, QR_v and T
PLANTING = [('U', np.nan, 1.5, 2.5), ('QR_v', np.nan, 4.0, 4.6), ('QR_v', 'neg', 5.5, 6.3), ('T', 330.0, 6.4, 6.9),
            ('T', 150.0, 7.0, 7.6), ('U', -9999.0, 8.5, 10.0), ('T', np.nan, 12.6, 13.0)]
CASES = list(S.ROUND_TRIP) + ['bench_c2']


def perturbed(cube, seed, plant=False):
    """A seeded other state of the same model: Q*_v scaled by 0.5 - 2 per variable, T 3 K colder (moves the melting layer and
    the tables' temperature bins), U and V swapped."""
    rng = np.random.default_rng(seed)
    data = {}
    for k in sorted(cube['data']):
        v = cube['data'][k]
        if k.startswith('Q') and k.endswith('_v'):
            data[k] = (v * np.float32(rng.uniform(0.5, 2.0))).astype(np.float32)
        elif k == 'T':
            data[k] = (v - np.float32(3.0)).astype(np.float32)
        else:
            data[k] = v
    data['U'], data['V'] = cube['data']['V'].copy(), cube['data']['U'].copy()
    out = dict(cube, data=data)
    if plant:
        out['data'] = {k: v.copy() for k, v in data.items()}
        GG.plant_bad_values(out, PLANTING)
    return out


@functools.lru_cache(maxsize=2)
def case(name):
    """(config, luts, [member cubes], azimuths, elevations)"""
    if name == 'bench_c2':
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import bench
        conf, hyds, cube, luts = bench.make_inputs('c2')
        az, el = np.arange(360.0), np.full(360, 1.0)
    else:
        _, a, e, _, luts, cube = _cases.radial_case(name)
        conf = GG.radial_case_inputs(name)[0]
        az, el = np.array([a, a + 0.5]), np.array([e, e])
    return conf, luts, [cube, perturbed(cube, 101), perturbed(cube, 202, plant=True)], az, el


def operator(conf, luts, **kw):
    from cosmo_pol_amd import RadarOperator
    return RadarOperator(config=copy.deepcopy(conf), luts=luts, output_variables='only_radar', **kw)


def load(op, cube):
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])


def ensemble_operator(name, **kw):
    conf, luts, cubes, az, el = case(name)
    op = operator(conf, luts, **kw)
    op.load_model_ensemble([c['data'] for c in cubes], cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    assert op.n_members == len(cubes)
    return op, az, el


@functools.lru_cache(maxsize=2)
def alone(name):
    """simulate_rays of a fresh operator loaded with member m alone, for every member (and its launch forms)."""
    conf, luts, cubes, az, el = case(name)
    out = []
    for cube in cubes:
        op = operator(conf, luts)
        load(op, cube)
        assert op.n_members == 1
        res = op.simulate_rays(az, el)
        out.append(({k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}, op._ctx.launch_forms()))
        op.close()
    return out


def assert_member_equals(got, m_row, ref, tag):
    """every output array of row `m_row` of an ensemble result == the single run's: dtype, shape, every gate"""
    n = 0
    for k in FIELDS:
        assert (k in got) == (k in ref), (tag, k)
        if k not in ref:
            continue
        a, b = got[k][m_row], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, k, a.dtype, b.dtype, a.shape, b.shape)
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        print('%s %s: %d of %d gates differ' % (tag, k, int((~same).sum()), same.size))
        assert np.array_equal(a, b, equal_nan=True), (tag, k, int((~same).sum()))
        n += 1
    assert n >= 10, (tag, n)                              # the 9 polarimetric fields and the mask at least
    for k in GEOM:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k], equal_nan=True), (tag, k)


@pytest.mark.parametrize('form', ['shared', 'per_member'])
@pytest.mark.parametrize('name', CASES)
def test_every_member_carries_the_bits_of_its_own_operator(name, form):
    op, az, el = ensemble_operator(name)
    refs = alone(name)
    got = op.simulate_rays_ensemble(az, el, form=form)
    forms = op._ctx.launch_forms()
    if form == 'shared':
        assert forms['interp_classify'] == 0 and forms['graph_replayed'] == 0
    for m, (ref, _) in enumerate(refs):
        assert_member_equals(got, m, ref, '%s/%s/member %d' % (name, form, m))
    # not a degenerate result
    zh = got['ZH']
    for m in range(3):
        assert np.isfinite(zh[m]).sum() > 0, m
    assert (~((zh[0] == zh[1]) | (np.isnan(zh[0]) & np.isnan(zh[1])))).sum() > 0
    assert (got['mask'][2] != got['mask'][0]).sum() > 0, 'the planted U of member 2 did not reach the mask'
    # a subset in another order
    sub = op.simulate_rays_ensemble(az, el, members=[2, 0], form=form)
    assert sub['ZH'].shape[0] == 2
    assert_member_equals(sub, 0, refs[2][0], 'subset row 0 = member 2')
    assert_member_equals(sub, 1, refs[0][0], 'subset row 1 = member 0')
    op.close()


def test_perturbed_members_keep_valid_gates_on_the_cpu_oracle():
    """The perturbations leave valid gates, and member 2's planting reaches the oracle's mask (one radial, no GPU result)."""
    conf, az, el, ocube, luts, cube = _cases.radial_case('c4_7x7')
    olut = {h: _cases.as_oracle_lut(l) for h, l in luts.items()}
    base = None
    for m, c in enumerate(case('c4_7x7')[2]):
        oc = beam.ModelCube({n: c['data'][n].copy() for n in _cases.ORDER}, c['zlevels'], c['proj_info'], c['resolution'],
                            _cases.ORDER)
        obs = scatter.radar_observables(beam.interpolate_radial(oc, conf, az, el), olut, conf)
        assert np.isfinite(obs.values['ZH']).sum() > 10, m
        if m == 0:
            base = obs
        elif m == 2:
            assert (obs.mask != base.mask).sum() > 0


def test_member_0_meets_the_golden_file_and_the_oracle(golden):
    name = 'c4_7x7'
    g = golden('radial_' + name)
    conf, az, el, ocube, luts, cube = _cases.radial_case(name)
    op, _, _ = ensemble_operator(name)
    res = op.simulate_rays_ensemble([az], [el], apply_sensitivity=False, form='shared')
    obs = types.SimpleNamespace(values={k: res[k][0][0] for k in S.OUT if k in res}, mask=res['mask'][0][0])
    assert np.array_equal(obs.mask, g['obs_mask'])
    for k in ['ZH', 'ZDR', 'RHOHV']:
        _cases.assert_close_nan(obs.values[k], g['obs_' + k], rtol=S.RTOL, name='golden:' + k)
    S._against_oracle(obs, beam.interpolate_radial(ocube, conf, az, el), luts, conf, name + ':')
    op.close()


def test_one_member_per_chunk_gives_the_bits_of_one_chunk():
    op, az, el = ensemble_operator('c4_7x7')
    one = op.simulate_rays_ensemble(az, el, form='shared')
    op.sequence_memory_budget = 1                         # no member fits: a chunk each
    cut = op.simulate_rays_ensemble(az, el, form='shared')
    for k in FIELDS + GEOM:
        if k in one:
            assert cut[k].shape == one[k].shape and np.array_equal(cut[k], one[k], equal_nan=True), k
    op.close()


@pytest.mark.parametrize('name', ['c4_7x7', 'bench_c2'])
def test_select_member(name, monkeypatch):
    """sweep, select_member(1), sweep == member 1 alone -- for the C2 sweep on its graph-replay path -- and back."""
    if name == 'bench_c2':
        monkeypatch.setenv('CPOL_USE_GRAPH', '1')
    op, az, el = ensemble_operator(name)
    refs = alone(name)
    import torch
    n_gates = refs[0][0]['ZH'].shape[1]
    dev = {k: torch.empty((len(az), n_gates), dtype=torch.float32, device='cuda') for k in ('ZH', 'KDP', 'PHIDP')}
    ptrs = {k: v.data_ptr() for k, v in dev.items()}

    def sweep():
        if name != 'bench_c2':
            return op.simulate_rays(az, el), 0
        replayed = 0
        for _ in range(3):                                # (device outputs, unchanged arguments: captured, then replayed)
            op.simulate_rays(az, el, device_outputs=ptrs)
            op.wait()
            replayed = op._ctx.launch_forms()['graph_replayed']
        return {k: v.cpu().numpy() for k, v in dev.items()}, replayed

    for m in (0, 1, 0, 2):
        op.select_member(m)
        got, replayed = sweep()
        if name == 'bench_c2':
            assert replayed == 1, 'the C2 sweep with device outputs no longer replays its graph'
        for k, v in got.items():
            if isinstance(v, np.ndarray) and k in refs[m][0]:
                assert np.array_equal(v, refs[m][0][k], equal_nan=True), (m, k)
    with pytest.raises(ValueError):
        op.select_member(3)
    op.close()


def test_existing_calls_behave_as_after_load_model_arrays():
    conf, luts, cubes, az, el = case('c4_7x7')
    op, _, _ = ensemble_operator('c4_7x7')
    plain = operator(conf, luts)
    load(plain, cubes[0])
    a, b = op.simulate_rays(az, el), plain.simulate_rays(az, el)
    assert op._ctx.launch_forms() == plain._ctx.launch_forms()
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(a[k], v, equal_nan=True), k
    pa, pb = op.get_PPI([1.0, 2.0], azimuths=[10.0, 11.0, 12.0]), plain.get_PPI([1.0, 2.0], azimuths=[10.0, 11.0, 12.0])
    assert op._ctx.launch_forms() == plain._ctx.launch_forms()
    for i in range(2):
        for k, v in pb.raw[i]['fields'].items():
            assert np.array_equal(np.asarray(pa.raw[i]['fields'][k]), np.asarray(v), equal_nan=True), (i, k)
    # the scan API of the ensemble: one RadarScan per member, member m's = get_PPI after select_member(m)
    scans = op.get_PPI_ensemble([1.0, 2.0], azimuths=[10.0, 11.0, 12.0])
    assert len(scans) == 3
    for m in (1, 2):
        op.select_member(m)
        want = op.get_PPI([1.0, 2.0], azimuths=[10.0, 11.0, 12.0])
        for i in range(2):
            for k, v in want.raw[i]['fields'].items():
                assert np.array_equal(np.asarray(scans[m].raw[i]['fields'][k]), np.asarray(v), equal_nan=True), (m, i, k)
            assert np.array_equal(scans[m].raw[i]['mask'], want.raw[i]['mask'])
    rhi = op.get_RHI_ensemble([30.0], elevations=[1.0, 2.0, 3.0], members=[1])
    assert len(rhi) == 1 and np.isfinite(np.asarray(rhi[0].raw[0]['fields']['ZH'])).sum() > 0
    op.close()
    plain.close()


def test_lane_and_pinned_outputs():
    op, az, el = ensemble_operator('c4_7x7')
    host = op.simulate_rays_ensemble(az, el, form='shared')
    lane = op.simulate_rays_ensemble(az, el, form='shared', lane=1, pinned=True)
    op.wait(1)
    for k in FIELDS + GEOM:
        if k in host:
            assert np.array_equal(lane[k], host[k], equal_nan=True), k
    import torch
    shape = host['ZH'].shape
    dev = {k: torch.empty(shape, dtype=torch.float32, device='cuda') for k in ('ZH', 'ZDR', 'PHIDP')}
    dev['mask'] = torch.empty(shape, dtype=torch.float64, device='cuda')
    op.simulate_rays_ensemble(az, el, form='shared', lane=1, device_outputs={k: v.data_ptr() for k, v in dev.items()})
    op.wait(1)
    for k, v in dev.items():
        assert np.array_equal(v.cpu().numpy(), host[k], equal_nan=True), k
    op.close()


def test_errors_leave_the_context_usable():
    conf, luts, cubes, az, el = case('c4_7x7')
    op, _, _ = ensemble_operator('c4_7x7')
    good = op.simulate_rays_ensemble(az, el, form='shared')
    with pytest.raises(ValueError):
        op.simulate_rays_ensemble(az, el, members=[0, 3])
    with pytest.raises(ValueError):
        op.simulate_rays_ensemble(az, el, members=[1, 1])
    # the library's own refusals (the context stays usable)
    with pytest.raises(ValueError):
        op._ctx.select_member(7)
    with pytest.raises(ValueError):
        op._ctx.stage_member(5, [cubes[1]['data'][k] for k in op._staged_vars])      # members are staged in order
    # rays that leave the model domain: IndexError once, then a correct call
    near = op.config
    far = op.config
    far['radar']['range'] = 150000                        # leaves the 1.1 deg test cube
    op.config = far
    assert op.n_members == 3                              # (a configuration that does not restage the cube keeps the members)
    with pytest.raises(IndexError):
        op.simulate_rays_ensemble(az, el, form='shared')
    op.wait()                                             # reported once, then cleared
    op.config = near
    again = op.simulate_rays_ensemble(az, el, form='shared')
    for k in FIELDS:
        if k in good:
            assert np.array_equal(again[k], good[k], equal_nan=True), k
    op.close()
    # antenna-integrated model variables are not part of an ensemble call
    from cosmo_pol_amd import RadarOperator
    full = RadarOperator(config=copy.deepcopy(conf), luts=luts, output_variables='all')
    full.load_model_ensemble([c['data'] for c in cubes], cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    with pytest.raises(NotImplementedError):
        full.simulate_rays_ensemble(az, el)
    full.close()


def test_members_cost_their_cube_and_give_it_back():
    conf, luts, cubes, az, el = case('c4_7x7')
    op = operator(conf, luts)
    load(op, cubes[0])
    op.simulate_rays(az, el)                              # (tables built, work buffers grown)
    names = op._staged_vars
    cube_bytes = sum(cubes[0]['data'][k].astype(np.float32).nbytes for k in names)
    free0 = op._ctx.mem_info()[0]
    op.load_model_ensemble([c['data'] for c in cubes], cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    free1 = op._ctx.mem_info()[0]
    print('two members of %d bytes each: free memory dropped by %d bytes' % (cube_bytes, free0 - free1))
    assert free0 - free1 >= 2 * cube_bytes
    load(op, cubes[0])                                    # a new load_model_*: the members go
    assert op.n_members == 1
    free2 = op._ctx.mem_info()[0]
    print('after restaging member 0 alone: %d bytes came back' % (free2 - free1))
    assert free2 - free1 >= 2 * cube_bytes
    op.close()
