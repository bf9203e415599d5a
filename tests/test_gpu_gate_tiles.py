"""k_gate1_ray on ray x gate tiles (cosmo_pol_amd/csrc/cpol_tile.h): the lanes path gives the bits of the one-lane path
(CPOL_GATE1_RAY=0: k_gate1_species + k_final) and of the general sequence (CPOL_GATE1=0) -- on the c2 sweep, on sweeps
whose ray and gate counts are not multiples of the tile, with items outside the integral tables (integrated in place),
with and without the sensitivity cut, RVEL included, and with three lanes in flight."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ('ZH', 'ZV', 'ZDR', 'RHOHV', 'KDP', 'PHIDP', 'DELTA_HV', 'ATT_H', 'ATT_V', 'RVEL', 'mask')
ENV_KEYS = ('CPOL_GATE1', 'CPOL_GATE1_RAY', 'CPOL_GATE1_SPECIES', 'CPOL_RARE_DIRECT', 'CPOL_ITAB_KEEP_PANELS')
MODES = (('ray', {'CPOL_GATE1_RAY': '1'}), ('onelane', {'CPOL_GATE1_RAY': '0'}), ('general', {'CPOL_GATE1': '0'}))


@pytest.fixture(scope='module')
def c2_inputs():
    import bench
    return bench.make_inputs('c2', False)


def _operator(monkeypatch, env, conf, luts, cube, lanes=1):
    from cosmo_pol_amd import RadarOperator
    for k in ENV_KEYS:
        if k not in env:
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                     # (read when the context is created)
    op = RadarOperator(config=conf, luts=luts, output_variables='only_radar', lanes=lanes)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    return op


def _check_form(mode, forms):
    if mode == 'ray':
        assert forms['gate1_ray'] == 1 and forms['gate1'] == 1, forms
    elif mode == 'onelane':
        assert forms['gate1_ray'] == 0 and forms['gate1'] == 1, forms
    else:
        assert forms['gate1'] == 0, forms


def _same(a, b, what):
    for k in FIELDS:
        assert a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, int((~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k])))).sum()))


def _three_ways(monkeypatch, conf, luts, cube, sweeps, extra_env=None, extra_modes=()):
    """sweeps: [(az, el, apply_sensitivity)] -> {mode: [result per sweep]}, every mode's launch form checked"""
    out = {}
    for mode, env in MODES + tuple(extra_modes):
        op = _operator(monkeypatch, dict(env, **(extra_env or {})), conf, luts, cube)
        out[mode] = []
        for az, el, sens in sweeps:
            out[mode].append(op.simulate_rays(az, el, apply_sensitivity=sens))
            _check_form('ray' if mode == 'ticket' else mode, op._ctx.launch_forms())
        op.close()
    return out


def test_c2_sweep_two_elevations_three_ways(monkeypatch, c2_inputs):
    import bench
    conf, hyds, cube, luts = c2_inputs
    az = np.arange(0, 360, 1.0)
    sweeps = [(az, np.full(360, el), True) for el in (bench.C2_ELEVATIONS[0], 1.35)]
    out = _three_ways(monkeypatch, conf, luts, cube, sweeps)
    assert out['ray'][0]['ZH'].shape == (360, 500)
    assert np.isfinite(out['ray'][0]['ZH']).sum() > 20000 and np.isfinite(out['ray'][0]['RVEL']).sum() > 20000
    for mode in ('onelane', 'general'):
        for s in range(len(sweeps)):
            _same(out['ray'][s], out[mode][s], (mode, s))


@pytest.mark.parametrize('n_rays,n_gates,rng,res', [(359, 497, 149100, 300), (17, 3, 5000, 1700), (1, 1, 5000, 5000)])
def test_sweeps_not_multiples_of_the_tile(monkeypatch, c2_inputs, n_rays, n_gates, rng, res):
    conf, hyds, cube, luts = c2_inputs
    conf = copy.deepcopy(conf)
    conf['radar'].update(range=rng, radial_resolution=res)      # (gates at res/2, 3 res/2, ... below the range; range >= 5 km)
    az = np.linspace(3.0, 3.0 + 0.997 * (n_rays - 1), n_rays)
    sweeps = [(az, np.full(n_rays, 1.0), True), (az, np.full(n_rays, 1.0), False), (az, np.full(n_rays, 1.2), True)]
    extra = (('ticket', {'CPOL_GATE1_RAY': '3'}),) if n_rays == 359 else ()
    out = _three_ways(monkeypatch, conf, luts, cube, sweeps, extra_modes=extra)
    assert out['ray'][0]['ZH'].shape == (n_rays, n_gates)
    if n_rays == 359:
        assert np.isfinite(out['ray'][1]['ZH']).sum() > 20000
        assert np.isnan(out['ray'][0]['ZH']).sum() > np.isnan(out['ray'][1]['ZH']).sum()      # (the cut took gates)
    for mode in ('onelane', 'general') + tuple(m for m, _ in extra):
        for s in range(len(sweeps)):
            _same(out['ray'][s], out[mode][s], (mode, n_rays, n_gates, s))


def test_items_outside_the_tables_on_tiles(monkeypatch):
    """Tables cut to their lower panels (CPOL_ITAB_KEEP_PANELS) and the path forced (CPOL_GATE1_RAY=2): the items off the
    tables are integrated in place by the wavefront of the tile that meets them (23 rays x 131 gates: partial tiles both
    ways), against the one-lane path (integrating launch + k_final) and the general sequence with the counting sort."""
    import bench
    from cosmo_pol_amd import synthetic
    hyds = ('R', 'S', 'G', 'H')
    cube = synthetic.small_test_cube(hydrometeors=('R', 'S', 'G'), two_moment=True)
    conf = bench.bench_config(True)
    conf['microphysics'].update(scheme='2mom', with_ice_crystals=0)
    conf['radar']['range'] = conf['radar']['radial_resolution'] * 131
    luts = synthetic.make_all_luts(hyds, 5.6, '2mom', n_e=8)
    op = _operator(monkeypatch, {}, conf, luts, cube)
    n_pan = [op._ctx.itab_detail(j)['n_pan'] for j in range(len(hyds))]
    op.close()
    keep = {'CPOL_ITAB_KEEP_PANELS': '0:%d' % (min(n_pan) * 5 // 8)}
    az = np.arange(20.0, 20.0 + 2.5 * 23, 2.5)
    sweeps = [(az, np.full(len(az), 2.0), True)]
    modes = (('ray', {'CPOL_GATE1_RAY': '2'}), ('onelane', {'CPOL_GATE1_RAY': '0'}),
             ('general', {'CPOL_GATE1': '0', 'CPOL_RARE_DIRECT': '0'}))
    out, counts = {}, {}
    for mode, env in modes:
        op = _operator(monkeypatch, dict(env, **keep), conf, luts, cube)
        out[mode] = op.simulate_rays(*sweeps[0][:2])
        _check_form(mode, op._ctx.launch_forms())
        c = op._ctx.counters()
        counts[mode] = (int(c.n_valid_items), int(c.n_table_items))
        op.close()
    assert counts['ray'] == counts['onelane'] == counts['general'], counts
    assert counts['ray'][0] - counts['ray'][1] > 50 and counts['ray'][1] > 50, counts     # items off the tables and on them
    assert out['ray']['ZH'].shape == (23, 131) and np.isfinite(out['ray']['ZH']).sum() > 300
    _same(out['ray'], out['onelane'], 'onelane')
    _same(out['ray'], out['general'], 'general')


def test_three_lanes_in_flight_against_one_lane(monkeypatch, c2_inputs):
    import torch
    import bench
    conf, hyds, cube, luts = c2_inputs
    conf = copy.deepcopy(conf)
    conf['radar']['range'] = conf['radar']['radial_resolution'] * 497
    n_rays, n_gates = 359, 497
    az = np.arange(0, n_rays, 1.0)
    els = [np.full(n_rays, e) for e in bench.C2_ELEVATIONS[:6]]
    op = _operator(monkeypatch, {}, conf, luts, cube, lanes=3)
    lanes = [op._lane(i) for i in range(3)]
    slabs = [torch.full((len(bench.RADAR_FIELDS), n_rays, n_gates), -7.0, dtype=torch.float32, device='cuda') for _ in els]
    rvel = [torch.full((n_rays, n_gates), -7.0, dtype=torch.float64, device='cuda') for _ in els]
    outs = [dict({k: sl[i].data_ptr() for i, k in enumerate(bench.RADAR_FIELDS)}, RVEL=rv.data_ptr()) for sl, rv in zip(slabs, rvel)]
    for k, el in enumerate(els):
        op.simulate_rays(az, el, device_outputs=outs[k], lane=k % 3)
        f = lanes[k % 3].launch_forms()
        assert f['gate1_ray'] == 1 and f['lanes_alive'] >= 2, f
    for i in range(3):
        op.wait(i)
    torch.cuda.synchronize()
    got = [sl.cpu().numpy() for sl in slabs]
    got_rvel = [rv.cpu().numpy() for rv in rvel]
    op.close()
    for mode, env in (('ray', {'CPOL_GATE1_RAY': '1'}), ('onelane', {'CPOL_GATE1_RAY': '0'})):
        op1 = _operator(monkeypatch, env, conf, luts, cube, lanes=1)
        for k, el in enumerate(els):
            one = op1.simulate_rays(az, el)
            _check_form(mode, op1._ctx.launch_forms())
            for i, f in enumerate(bench.RADAR_FIELDS):
                assert np.array_equal(one[f], got[k][i], equal_nan=True), (mode, f, k)
            assert np.array_equal(one['RVEL'], got_rvel[k], equal_nan=True), (mode, 'RVEL', k)
        op1.close()
    assert np.isfinite(got[0][0]).sum() > 20000
