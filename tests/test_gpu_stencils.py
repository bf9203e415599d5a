"""Gate stencils (cosmo_pol_amd/csrc/cpol_interp.inl: k_interp_record / k_interp_replay): a single-beam sweep of a geometry seen
before replays what its gates knew before they read the model's values.  Every result here is compared, bit for bit
(np.array_equal with equal_nan on the nine observables, RVEL and mask), with an operator whose stencils are off
(stencil_budget=0): the life cycle noted -> recording -> replay, every geometric class of gate, the mask born from the data,
what invalidates a stencil and what does not, lanes, and the memory budget."""
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


def _sweep(op, az, el, sens=True, lane=0, raises=False):
    """-> (the eleven arrays, the form the sweep took)"""
    slab = _Slab(len(az), _n_gates(op))
    op.simulate_rays(az, el, device_outputs=slab.ptrs, apply_sensitivity=sens, lane=lane)
    form = op.stencil_state(lane)['form']
    if raises:
        with pytest.raises(IndexError):
            op.wait(lane)
    else:
        op.wait(lane)
    return slab.numpy(), form


def _same(a, b, what, where=None):
    assert sorted(a) == sorted(b) and len(a) == 11
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        x, y = (a[k], b[k]) if where is None else (a[k][where], b[k][where])
        assert np.array_equal(x, y, equal_nan=True), (what, k, int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum()))


def _rays(n, el):
    return np.linspace(3.0, 3.0 + 0.997 * (n - 1), n) if n > 1 else np.array([3.0]), np.full(n, float(el))


# ---------------------------------------------------------------- 1. the life cycle
@pytest.mark.parametrize('sens', [True, False])
@pytest.mark.parametrize('n_rays,n_gates,rng,res', [(17, 100, 30000, 300), (1, 1, 5000, 5000), (65, 257, 25700, 100)])
def test_life_cycle_gives_the_full_forms_bits(inputs, n_rays, n_gates, rng, res, sens):
    conf, cube, luts = inputs
    conf = copy.deepcopy(conf)
    conf['radar'].update(range=rng, radial_resolution=res)
    az, el = _rays(n_rays, 2.0)
    base = _operator(conf, luts, cube, budget=0)
    want, form = _sweep(base, az, el, sens)
    assert form == FULL and want['ZH'].shape == (n_rays, n_gates)
    _same(_sweep(base, az, el, sens)[0], want, 'baseline again')
    assert base.stencil_state()['entries'] == 0
    base.close()
    if n_gates > 1:
        assert np.isfinite(want['ZH']).sum() > n_rays * n_gates // 10
    op = _operator(conf, luts, cube)
    forms = []
    for k in range(4):
        got, form = _sweep(op, az, el, sens)
        forms.append(form)
        _same(got, want, 'sweep %d (form %d)' % (k, form))
    assert forms == [FULL, RECORDING, REPLAY, REPLAY]
    st = op.stencil_state()
    assert st['entries'] == 1 and st['records'] == 1 and st['replays'] == 2 and st['drops'] == 0
    assert st['bytes'] == 69 * ((n_rays * n_gates + 63) // 64 * 64)
    op.close()


# ---------------------------------------------------------------- 2. every geometric class
def test_every_geometric_class_replays(inputs):
    """Rays into the ground, rays at 1 degree, and rays steep enough to leave the model through its top, in one sweep."""
    conf, cube, luts = inputs
    conf = copy.deepcopy(conf)
    conf['radar'].update(range=60000, radial_resolution=600)
    az = np.arange(10.0, 10.0 + 12 * 29.0, 29.0)
    el = np.tile([-4.0, 1.0, 60.0, 25.0], 3)
    base = _operator(conf, luts, cube, budget=0)
    want, _ = _sweep(base, az, el, False)
    base.close()
    m = want['mask']
    assert (m < 0).sum() > 20 and (m > 0).sum() > 20 and (m == 0).sum() > 100, [(m < 0).sum(), (m > 0).sum(), (m == 0).sum()]
    op = _operator(conf, luts, cube)
    forms = []
    for k in range(4):
        got, form = _sweep(op, az, el, False)
        forms.append(form)
        _same(got, want, 'sweep %d' % k)
    assert forms == [FULL, RECORDING, REPLAY, REPLAY]
    op.close()


def test_gates_outside_the_domain_raise_on_every_replay(inputs):
    conf, cube, luts = inputs
    conf = copy.deepcopy(conf)
    conf['radar'].update(range=90000, radial_resolution=900)        # the cube reaches ~61 km from the radar
    az, el = _rays(17, 1.5)
    base = _operator(conf, luts, cube, budget=0)
    want, _ = _sweep(base, az, el, True, raises=True)
    base.close()
    inside = want['mask'] != 2
    assert (~inside).sum() > 17 * 10 and inside.sum() > 17 * 50 and np.isfinite(want['ZH'][inside]).sum() > 100
    op = _operator(conf, luts, cube)
    forms = []
    for k in range(4):
        got, form = _sweep(op, az, el, True, raises=True)         # (the same IndexError on the first call and on a replayed one)
        forms.append(form)
        _same(got, want, 'sweep %d' % k)
        _same(got, want, 'sweep %d, inside' % k, where=inside)
    assert forms == [FULL, RECORDING, REPLAY, REPLAY]
    op.close()


# ---------------------------------------------------------------- 3. the mask born from data
def _planted(cube, var0):
    """NaN and -9999 in variable 0 and NaN in T, in rings of grid columns around the radar (as the bad_* cases plant them)."""
    data = {k: v.copy() for k, v in cube['data'].items()}
    ny, nx = data['T'].shape[1:]
    yy, xx = np.meshgrid(np.arange(ny) - (ny - 1) / 2., np.arange(nx) - (nx - 1) / 2., indexing='ij')
    r = np.hypot(yy, xx)
    for var, value, lo, hi in ((var0, np.nan, 1.5, 2.5), (var0, -9999.0, 6.5, 9.5), ('T', np.nan, 11.0, 11.6)):
        data[var][:, (r >= lo) & (r < hi)] = np.float32(value)
    return dict(cube, data=data)


def test_mask_born_from_data_is_not_in_the_record(inputs):
    conf, cube, luts = inputs
    az, el = _rays(17, 4.0)
    op = _operator(conf, luts, cube)
    clean = [_sweep(op, az, el) for _ in range(3)]
    assert [f for _, f in clean] == [FULL, RECORDING, REPLAY]
    bad = _planted(cube, op._staged_vars[0])
    op.load_model_arrays(bad['data'], bad['zlevels'], bad['proj_info'], bad['resolution'])
    got, form = _sweep(op, az, el)
    assert form == REPLAY and op.stencil_state()['drops'] == 0
    op.close()
    base = _operator(conf, luts, bad, budget=0)
    want, _ = _sweep(base, az, el)
    base.close()
    _same(got, want, 'planted')
    # the planting reached the sweep: gates masked by the data, with either sign
    assert (want['mask'] > 0).sum() > (clean[0][0]['mask'] > 0).sum() + 10
    assert (want['mask'] < 0).sum() > (clean[0][0]['mask'] < 0).sum() + 10


# ---------------------------------------------------------------- 4. invalidation
def _recorded(conf, luts, cube, az, el, sens=True):
    op = _operator(conf, luts, cube)
    assert [_sweep(op, az, el, sens)[1] for _ in range(3)] == [FULL, RECORDING, REPLAY]
    return op


def _fresh(conf, luts, cube, az, el, sens=True):
    base = _operator(conf, luts, cube, budget=0)
    want, _ = _sweep(base, az, el, sens)
    base.close()
    return want


def test_equal_heights_keep_the_stencils(inputs):
    conf, cube, luts = inputs
    az, el = _rays(17, 3.0)
    op = _recorded(conf, luts, cube, az, el)
    other = dict(cube, data={k: (v * np.float32(0.5) if k.startswith('Q') else v + np.float32(0.25)) for k, v in cube['data'].items()},
                 zlevels=cube['zlevels'].copy())
    op.load_model_arrays(other['data'], other['zlevels'], other['proj_info'], other['resolution'])
    st = op.stencil_state()
    assert st['entries'] == 1 and st['drops'] == 0
    got, form = _sweep(op, az, el)
    assert form == REPLAY
    op.close()
    want = _fresh(conf, luts, other, az, el)
    _same(got, want, 'other values')
    assert not np.array_equal(want['ZH'], _fresh(conf, luts, cube, az, el)['ZH'], equal_nan=True)


def test_one_ulp_in_one_level_drops_them(inputs):
    conf, cube, luts = inputs
    az, el = _rays(17, 3.0)
    op = _recorded(conf, luts, cube, az, el)
    z = cube['zlevels'].copy()
    nz, ny, nx = z.shape
    z[nz // 2, ny // 2 + 3, nx // 2 + 2] = np.nextafter(z[nz // 2, ny // 2 + 3, nx // 2 + 2], np.float32(np.inf))
    assert (z != cube['zlevels']).sum() == 1
    moved = dict(cube, zlevels=z)
    op.load_model_arrays(moved['data'], moved['zlevels'], moved['proj_info'], moved['resolution'])
    st = op.stencil_state()
    assert st['entries'] == 0 and st['drops'] == 1 and st['bytes'] == 0
    forms = []
    want = _fresh(conf, luts, moved, az, el)
    for k in range(3):
        got, form = _sweep(op, az, el)
        forms.append(form)
        _same(got, want, 'moved level, sweep %d' % k)
    assert forms == [FULL, RECORDING, REPLAY]
    op.close()


def test_another_pole_or_level_count_drops_them(inputs):
    conf, cube, luts = inputs
    az, el = _rays(17, 3.0)
    op = _recorded(conf, luts, cube, az, el)
    turned = dict(cube, proj_info=dict(cube['proj_info'],
                                       Latitude_of_southern_pole=cube['proj_info']['Latitude_of_southern_pole'] + 0.01))
    op.load_model_arrays(turned['data'], turned['zlevels'], turned['proj_info'], turned['resolution'])
    st = op.stencil_state()
    assert st['entries'] == 0 and st['drops'] == 1
    want = _fresh(conf, luts, turned, az, el)
    forms = []
    for k in range(3):
        got, form = _sweep(op, az, el)
        forms.append(form)
        _same(got, want, 'another pole, sweep %d' % k)
    assert forms == [FULL, RECORDING, REPLAY]
    # ... and one level less: the same grid, the same pole
    lower = dict(turned, data={k: np.ascontiguousarray(v[1:]) for k, v in turned['data'].items()},
                 zlevels=np.ascontiguousarray(turned['zlevels'][1:]))
    op.load_model_arrays(lower['data'], lower['zlevels'], lower['proj_info'], lower['resolution'])
    st = op.stencil_state()
    assert st['entries'] == 0 and st['drops'] == 2
    want = _fresh(conf, luts, lower, az, el)
    forms = []
    for k in range(3):
        got, form = _sweep(op, az, el)
        forms.append(form)
        _same(got, want, 'nz - 1, sweep %d' % k)
    assert forms == [FULL, RECORDING, REPLAY]
    op.close()


def test_same_table_version_another_range_grid_is_another_key(inputs):
    conf, cube, luts = inputs
    az, el = _rays(17, 3.0)
    # (without the sensitivity cut: its threshold table depends on the range grid and travels under the version tag)
    op = _recorded(conf, luts, cube, az, el, sens=False)
    rays = {k: v for k, v in op._cache.items() if isinstance(k, tuple) and k[0] == 'rays'}
    assert len(rays) == 1
    conf2 = copy.deepcopy(conf)
    conf2['radar'].update(range=15000, radial_resolution=150)      # 100 gates again: the table set's shape stays
    op.config = conf2
    op._cache.update(rays)                                         # (the per-ray tables keep their version tag)
    want = _fresh(conf2, luts, cube, az, el, sens=False)
    forms = []
    for k in range(3):
        got, form = _sweep(op, az, el, False)
        forms.append(form)
        _same(got, want, 'other range grid, sweep %d' % k)
    assert forms == [FULL, RECORDING, REPLAY]
    assert [k for k in op._cache if isinstance(k, tuple) and k[0] == 'rays'] == list(rays)
    st = op.stencil_state()
    assert st['entries'] == 2 and st['records'] == 2 and st['drops'] == 0
    op.close()
    assert not np.array_equal(want['ZH'], _fresh(conf, luts, cube, az, el, sens=False)['ZH'], equal_nan=True)


def test_members_share_a_stencil(inputs):
    conf, cube, luts = inputs
    az, el = _rays(17, 3.0)
    second = {k: (v * np.float32(0.25) if k.startswith('Q') else v - np.float32(0.5)) for k, v in cube['data'].items()}
    op = _operator(conf, luts, cube)
    op.load_model_ensemble([cube['data'], second], cube['zlevels'], cube['proj_info'], cube['resolution'])
    assert [_sweep(op, az, el)[1] for _ in range(3)] == [FULL, RECORDING, REPLAY]
    want = [_fresh(conf, luts, cube, az, el), _fresh(conf, luts, dict(cube, data=second), az, el)]
    assert not np.array_equal(want[0]['ZH'], want[1]['ZH'], equal_nan=True)
    for m in (1, 0, 1):
        op.select_member(m)
        got, form = _sweep(op, az, el)
        assert form == REPLAY
        _same(got, want[m], 'member %d' % m)
    assert op.stencil_state()['records'] == 1
    op.close()


# ---------------------------------------------------------------- 5. lanes
def test_three_lanes_share_the_store_and_it_outlives_them(inputs):
    import bench
    conf, cube, luts = inputs
    n_rays, n_lanes, n_cycle = 17, 3, 8
    az = _rays(n_rays, 0)[0]
    els = [np.full(n_rays, e) for e in bench.C2_ELEVATIONS[:n_cycle]]
    base = _operator(conf, luts, cube, budget=0, lanes=n_lanes)
    [base._lane(i) for i in range(n_lanes)]                      # (the lanes path on both sides: k_gate1_ray)
    want = [_sweep(base, az, e, lane=1)[0] for e in els]
    base.close()
    op = _operator(conf, luts, cube, lanes=n_lanes)
    [op._lane(i) for i in range(n_lanes)]
    slabs, forms = [], []
    for k in range(48):
        slabs.append(_Slab(n_rays, _n_gates(op)))
        op.simulate_rays(az, els[k % n_cycle], device_outputs=slabs[k].ptrs, lane=k % n_lanes)
        forms.append(op.stencil_state(k % n_lanes)['form'])
    for i in range(n_lanes):
        op.wait(i)
    assert forms == [FULL] * 8 + [RECORDING] * 8 + [REPLAY] * 32
    for k in range(48):
        _same(slabs[k].numpy(), want[k % n_cycle], 'sweep %d' % k)
    st = op.stencil_state()
    assert st['records'] == 8 and st['entries'] == 8 and st['replays'] == 32
    # the model again, with equal heights: the lanes are dropped and forked anew, the store stays
    op.load_model_arrays(cube['data'], cube['zlevels'].copy(), cube['proj_info'], cube['resolution'])
    assert op.stencil_state()['entries'] == 8
    [op._lane(i) for i in range(n_lanes)]
    for i in range(n_lanes):
        got, form = _sweep(op, az, els[i + 2], lane=i)
        assert form == REPLAY, (i, form)
        _same(got, want[i + 2], 'after the reload, lane %d' % i)
    st = op.stencil_state()
    assert st['records'] == 8 and st['drops'] == 0
    op.close()


# ---------------------------------------------------------------- 6. the budget
def test_budget(inputs):
    conf, cube, luts = inputs
    n_rays = 17
    az = _rays(n_rays, 0)[0]
    els = [np.full(n_rays, e) for e in (2.0, 3.0, 4.0)]
    base = _operator(conf, luts, cube, budget=0)
    want = [_sweep(base, az, e)[0] for e in els]
    base.close()
    one = 69 * ((n_rays * 100 + 63) // 64 * 64)
    op = _operator(conf, luts, cube, budget=one - 1)           # below one record
    for k in range(4):
        got, form = _sweep(op, az, els[0])
        assert form == FULL
        _same(got, want[0], 'no room, sweep %d' % k)
    assert op.stencil_state()['bytes'] == 0 and op.stencil_state()['records'] == 0
    op.close()
    op = _operator(conf, luts, cube, budget=3 * one - 1, lanes=2)       # room for two records, three geometries
    forms = []
    for k in range(12):
        got, form = _sweep(op, az, els[k % 3])
        forms.append(form)
        _same(got, want[k % 3], 'two of three, sweep %d' % k)
    assert forms == [FULL] * 3 + [RECORDING, RECORDING, FULL] + [REPLAY, REPLAY, FULL] * 2
    st = op.stencil_state()
    assert st['bytes'] == 2 * one and st['records'] == 2
    op._lane(1)                                                 # a lane exists: the budget stays what it is
    with pytest.raises(ValueError, match='lanes'):
        op._ctx.set_stencil_budget(0)
    assert op.stencil_state()['bytes'] == 2 * one
    op._drop_lanes()
    op._ctx.set_stencil_budget(0)                               # no lanes: lowered, every entry dropped
    st = op.stencil_state()
    assert st['bytes'] == 0 and st['entries'] == 0 and st['drops'] == 3
    got, form = _sweep(op, az, els[0])
    assert form == FULL
    _same(got, want[0], 'stencils off')
    op.close()
