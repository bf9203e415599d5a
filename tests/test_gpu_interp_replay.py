"""The replayed gate interpolation with a compile-time variable count (cosmo_pol_amd/csrc/cpol_interp.inl: k_interp_replay_n,
replay_gate): the whole record in one memory round, every model value of the gate in one more (two for the 2-moment cubes), the
statements of gate_value4 / gate_value behind them.  Only the order of the requests changed, so every sweep that replays is
compared BIT FOR BIT (np.array_equal with equal_nan) with an operator that never replays (stencil_budget=0): the eleven output
arrays and, through debug_read, what the interpolation itself leaves behind -- sub_values (every variable), sub_mask, sub_elev.
(The debug reads are taken WITHOUT enable_debug: with it the launch rules keep the float64 coordinates and the stencils are off,
cpol_forms.h.)

Variable counts.  The library has instantiations for 9 and 10 variables (one gather round) and for 15 and 16 (two rounds of eight
variables); every other count keeps k_interp_replay's run-time loop.  The operator stages 9 (1-moment), 10 (with EDR), 15
(2-moment) or 16 variables; the other counts are reached here by appending filler variables to the staged list (the indices of the
nine base variables stay what they are, as with EDR).  8, the count below the first instantiation, cannot be reached: the nine base
variables are always staged."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL, RECORDING, REPLAY = 0, 1, 2


@pytest.fixture(scope='module')
def inputs():
    import bench
    conf, hyds, cube, luts = bench.make_inputs('c2', True)          # the 56 x 56 x 30 cube, 100 gates of 300 m
    return conf, cube, luts


def _operator(conf, luts, cube, budget=None, lanes=1):
    from cosmo_pol_amd import RadarOperator
    op = RadarOperator(config=copy.deepcopy(conf), luts=luts, output_variables='only_radar', lanes=lanes, stencil_budget=budget)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    return op


class _Slab(object):
    """The outputs of one sweep in device memory (bench.py's step_hbm pattern)."""

    def __init__(self, n_rays, n_gates):
        import torch
        import bench
        self.f32 = torch.full((len(bench.RADAR_FIELDS), n_rays, n_gates), -7.0, dtype=torch.float32, device='cuda')
        self.f64 = torch.full((2, n_rays, n_gates), -7.0, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()                                    # (the fill is on another stream than the library's)
        self.ptrs = dict({k: self.f32[i].data_ptr() for i, k in enumerate(bench.RADAR_FIELDS)},
                         RVEL=self.f64[0].data_ptr(), mask=self.f64[1].data_ptr())

    def numpy(self):
        import torch
        import bench
        torch.cuda.synchronize()
        a, b = self.f32.cpu().numpy(), self.f64.cpu().numpy()
        return dict({k: a[i] for i, k in enumerate(bench.RADAR_FIELDS)}, RVEL=b[0], mask=b[1])


def _n_gates(op):
    return len(op.constants.RANGE_RADAR)


def _interp(op, n_rays, lane=0):
    """What the gate interpolation of the lane's last sweep left: values of every variable, mask, folded elevation."""
    ctx = op._lane(lane)
    n = n_rays * _n_gates(op)
    return {'sub_values': ctx.debug_read('sub_values', (len(op._staged_vars), n), np.float32),
            'sub_mask': ctx.debug_read('sub_mask', (n,), np.int8),
            'sub_elev': ctx.debug_read('sub_elev', (n,), np.float32)}


def _sweep(op, az, el, sens=True, lane=0, raises=False):
    """-> (the eleven arrays + the three of the interpolation, the form the sweep took)"""
    slab = _Slab(len(az), _n_gates(op))
    op.simulate_rays(az, el, device_outputs=slab.ptrs, apply_sensitivity=sens, lane=lane)
    form = op.stencil_state(lane)['form']
    if raises:
        with pytest.raises(IndexError):
            op.wait(lane)
    else:
        op.wait(lane)
    return dict(slab.numpy(), **_interp(op, len(az), lane)), form


def _same(a, b, what):
    assert sorted(a) == sorted(b) and len(a) == 14
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        x, y = a[k], b[k]
        assert np.array_equal(x, y, equal_nan=True), (what, k, int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum()))


def _rays(n, el):
    return np.linspace(3.0, 3.0 + 0.997 * (n - 1), n) if n > 1 else np.array([3.0]), np.full(n, float(el))


def _fresh(conf, luts, cube, az, el, sens=True, raises=False):
    base = _operator(conf, luts, cube, budget=0)
    want, form = _sweep(base, az, el, sens, raises=raises)
    assert form == FULL
    base.close()
    return want


def _replays(conf, luts, cube, az, el, want, what, sens=True, raises=False):
    """Four sweeps of one geometry: full, recording, and two replays, each with the baseline's bits.  -> the operator, open."""
    op = _operator(conf, luts, cube)
    forms = []
    for k in range(4):
        got, form = _sweep(op, az, el, sens, raises=raises)
        forms.append(form)
        _same(got, want, '%s, sweep %d (form %d)' % (what, k, form))
    assert forms == [FULL, RECORDING, REPLAY, REPLAY]
    return op


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize('n_rays,n_gates,rng,res', [(1, 1, 5000, 5000), (3, 65, 19500, 300), (5, 257, 25700, 100)])
def test_shapes(inputs, n_rays, n_gates, rng, res):
    """One gate; one lane past a wavefront; gate 256 in the second workgroup of a ray, 255 lanes of which return before any load."""
    conf, cube, luts = inputs
    conf = copy.deepcopy(conf)
    conf['radar'].update(range=rng, radial_resolution=res)
    az, el = _rays(n_rays, 2.0)
    want = _fresh(conf, luts, cube, az, el)
    assert want['ZH'].shape == (n_rays, n_gates) and want['sub_values'].shape == (9, n_rays * n_gates)
    if n_gates > 1:
        assert (want['sub_mask'] == 0).sum() > n_rays * n_gates // 2
    _replays(conf, luts, cube, az, el, want, 'shape').close()


# ---------------------------------------------------------------- 2. every geometric class, gates outside the domain
def test_every_geometric_class(inputs):
    """Rays into the ground, at 1 degree, and out through the model top in one sweep: the rows of the record that were never
    written for the gates above / below the model are loaded and must change nothing."""
    conf, cube, luts = inputs
    conf = copy.deepcopy(conf)
    conf['radar'].update(range=60000, radial_resolution=600)
    az = np.arange(10.0, 10.0 + 12 * 29.0, 29.0)
    el = np.tile([-4.0, 1.0, 60.0, 25.0], 3)
    want = _fresh(conf, luts, cube, az, el, sens=False)
    m = want['sub_mask']
    assert (m < 0).sum() > 20 and (m > 0).sum() > 20 and (m == 0).sum() > 100, [(m < 0).sum(), (m > 0).sum(), (m == 0).sum()]
    assert np.isnan(want['sub_values'][:, m != 0]).all() and np.isfinite(want['sub_values'][:, m == 0]).all()
    _replays(conf, luts, cube, az, el, want, 'classes', sens=False).close()


def test_gates_outside_the_domain_raise_on_every_replay(inputs):
    conf, cube, luts = inputs
    conf = copy.deepcopy(conf)
    conf['radar'].update(range=90000, radial_resolution=900)        # the cube reaches ~61 km from the radar
    az, el = _rays(17, 1.5)
    want = _fresh(conf, luts, cube, az, el, raises=True)
    outside = want['sub_mask'] == 2
    assert outside.sum() > 17 * 10 and (~outside).sum() > 17 * 50 and np.isnan(want['sub_values'][:, outside]).all()
    _replays(conf, luts, cube, az, el, want, 'outside', raises=True).close()


# ---------------------------------------------------------------- 3. the mask born from the values
def _planted(cube, var0):
    """-9999 in a ring of grid columns three cells wide (gates with all eight neighbours -9999, and gates at its edges), NaN in a
    ring one cell wide, both in variable 0; NaN in T further out."""
    data = {k: v.copy() for k, v in cube['data'].items()}
    ny, nx = data['T'].shape[1:]
    yy, xx = np.meshgrid(np.arange(ny) - (ny - 1) / 2., np.arange(nx) - (nx - 1) / 2., indexing='ij')
    r = np.hypot(yy, xx)
    for var, value, lo, hi in ((var0, np.nan, 1.5, 2.5), (var0, -9999.0, 6.5, 9.5), ('T', np.nan, 11.0, 11.6)):
        data[var][:, (r >= lo) & (r < hi)] = np.float32(value)
    return dict(cube, data=data)


def test_sentinels_in_variable_0(inputs):
    conf, cube, luts = inputs
    az, el = _rays(17, 4.0)
    clean = _fresh(conf, luts, cube, az, el)
    op = _replays(conf, luts, cube, az, el, clean, 'clean')
    bad = _planted(cube, op._staged_vars[0])
    op.load_model_arrays(bad['data'], bad['zlevels'], bad['proj_info'], bad['resolution'])
    got, form = _sweep(op, az, el)
    assert form == REPLAY and op.stencil_state()['drops'] == 0
    op.close()
    want = _fresh(conf, luts, bad, az, el)
    _same(got, want, 'planted')
    inside = clean['sub_mask'] == 0
    m, v0 = want['sub_mask'], want['sub_values'][0]
    # all eight neighbours -9999: masked +1 by the value; a NaN neighbour: masked -1; at the edge of the -9999 block: a huge
    # negative value that is neither, the gate stays valid
    assert (inside & (m == 1)).sum() > 10 and (inside & (m == -1)).sum() > 10
    assert (inside & (m == 0) & (v0 < -100.0)).sum() > 5
    assert np.isnan(want['sub_values'][:, inside & (m != 0)]).all()
    # NaN in T alone: the mask stays 0, the value travels
    assert (inside & (m == 0) & np.isnan(want['sub_values'][op._staged_vars.index('T')])).sum() > 5


# ---------------------------------------------------------------- 4. variable counts
def _with_fillers(monkeypatch, cube, n_fill):
    """The cube with n_fill more variables, and the staged list extended by them (behind the configuration's own)."""
    from cosmo_pol_amd import hydrometeors as hyd
    names = ['FILL%02d' % i for i in range(n_fill)]
    rng = np.random.default_rng(20261021)
    data = dict(cube['data'])
    for i, k in enumerate(names):
        data[k] = (cube['data']['T'] * np.float32(1.0 + 0.01 * i) + rng.random(cube['data']['T'].shape, dtype=np.float32)).astype(np.float32)
    plain = hyd.variable_list
    monkeypatch.setattr(hyd, 'variable_list', lambda config: plain(config) + names)
    return dict(cube, data=data)


@pytest.mark.parametrize('n_vars', [10, 11, 14, 15, 16, 17, 24])
def test_variable_counts(inputs, monkeypatch, n_vars):
    """9: every other test.  10 | 11 and 14 | 15, 16 | 17: the edges of the instantiation list (9, 10, 15, 16; 15 and 16 in rounds
    of 8 + 7 and 8 + 8 variables); 24: the library's largest cube.  The fillers hold data of their own, so a variable read from a
    wrong offset of the run shows."""
    conf, cube, luts = inputs
    cube = _with_fillers(monkeypatch, cube, n_vars - 9)
    az, el = _rays(3, 2.0)
    conf = copy.deepcopy(conf)
    conf['radar'].update(range=19500, radial_resolution=300)        # 65 gates
    want = _fresh(conf, luts, cube, az, el)
    assert want['sub_values'].shape == (n_vars, 3 * 65)
    ok = want['sub_mask'] == 0
    assert ok.sum() > 100 and np.isfinite(want['sub_values'][:, ok]).all()
    assert len(np.unique(want['sub_values'][9:, ok], axis=0)) == n_vars - 9
    _replays(conf, luts, cube, az, el, want, '%d variables' % n_vars).close()


def test_two_moment_cube(inputs):
    """The 15 variables of a 2-moment cube as the operator itself stages them."""
    import bench
    from cosmo_pol_amd import synthetic
    hyds = ('R', 'S', 'G', 'H')
    cube = synthetic.small_test_cube(hydrometeors=('R', 'S', 'G'), two_moment=True)
    conf = bench.bench_config(True)
    conf['microphysics'].update(scheme='2mom', with_ice_crystals=0)
    conf['radar']['range'] = conf['radar']['radial_resolution'] * 65
    luts = synthetic.make_all_luts(hyds, 5.6, '2mom', n_e=8)
    az, el = _rays(3, 2.0)
    want = _fresh(conf, luts, cube, az, el)
    assert want['sub_values'].shape == (15, 3 * 65) and np.isfinite(want['ZH']).sum() > 30
    _replays(conf, luts, cube, az, el, want, '2-moment').close()


# ---------------------------------------------------------------- 5. another cube between two replays
def test_a_cube_replaced_between_two_replays(inputs):
    conf, cube, luts = inputs
    az, el = _rays(17, 3.0)
    want = _fresh(conf, luts, cube, az, el)
    op = _replays(conf, luts, cube, az, el, want, 'first cube')
    other = dict(cube, data={k: (v * np.float32(0.5) if k.startswith('Q') else v + np.float32(0.25)) for k, v in cube['data'].items()},
                 zlevels=cube['zlevels'].copy())
    op.load_model_arrays(other['data'], other['zlevels'], other['proj_info'], other['resolution'])
    st = op.stencil_state()
    assert st['entries'] == 1 and st['drops'] == 0
    got, form = _sweep(op, az, el)
    assert form == REPLAY
    op.close()
    want2 = _fresh(conf, luts, other, az, el)
    _same(got, want2, 'second cube')
    assert not np.array_equal(want2['sub_values'], want['sub_values'], equal_nan=True)


# ---------------------------------------------------------------- 6. lanes
def test_three_lanes_alternate_over_two_geometries(inputs):
    conf, cube, luts = inputs
    n_rays, n_lanes = 5, 3
    az = _rays(n_rays, 0)[0]
    els = [np.full(n_rays, e) for e in (1.0, 8.0)]
    base = _operator(conf, luts, cube, budget=0, lanes=n_lanes)
    [base._lane(i) for i in range(n_lanes)]                      # (the lanes path on both sides)
    want = [_sweep(base, az, e, lane=1)[0] for e in els]
    base.close()
    op = _operator(conf, luts, cube, lanes=n_lanes)
    [op._lane(i) for i in range(n_lanes)]
    slabs, forms = [], []
    for k in range(14):
        slabs.append(_Slab(n_rays, _n_gates(op)))
        op.simulate_rays(az, els[k % 2], device_outputs=slabs[k].ptrs, lane=k % n_lanes)
        forms.append(op.stencil_state(k % n_lanes)['form'])
    for i in range(n_lanes):
        op.wait(i)
    assert forms == [FULL] * 2 + [RECORDING] * 2 + [REPLAY] * 10
    for k in range(14):
        got = slabs[k].numpy()
        for name in got:
            assert np.array_equal(got[name], want[k % 2][name], equal_nan=True), (k, name)
    # the last sweep of every lane (sweeps 11, 12, 13: lanes 2, 0, 1) left its interpolation in the lane's own buffers
    for k in (11, 12, 13):
        left = _interp(op, n_rays, k % n_lanes)
        for name in left:
            assert np.array_equal(left[name], want[k % 2][name], equal_nan=True), (k, name)
    op.close()
