"""k_gate1_ray and the wave slots of its empty wavefronts (cosmo_pol_amd/csrc/cpol_gate.inl): the wavefront of a species that
its tile does not hold returns behind the presence test, the wavefronts of the species present share the ticket among
themselves, a tile of clear air is finished by wavefront 0 alone.  Which wavefront finishes a tile must not show in a single
bit: the lanes path (CPOL_GATE1_RAY=1) is compared with the general sequence (CPOL_GATE1=0) on the nine observables, RVEL
and the mask through their uint32 / uint64 views (NaN payloads count), on 5 rays x 70 gates -- a padding ray, padding gates,
two presence words per ray -- for cubes whose mass densities put every kind of tile in front of the kernel, with and without
attenuation, with and without RVEL among the outputs, four sweeps in a row on one context (full form, recording, replay,
replay: the presence words of the replaying kernel are the ones read), and against a child process whose CPOL_GATE1_PRESENT=0
takes the all-present path on the same inputs."""
import contextlib
import copy
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_RAYS, N_GATES, RES = 5, 70, 300
ENV_KEYS = ('CPOL_GATE1', 'CPOL_GATE1_RAY', 'CPOL_GATE1_SPECIES', 'CPOL_RARE_DIRECT', 'CPOL_ITAB_KEEP_PANELS')
LANES, GENERAL = {'CPOL_GATE1_RAY': '1'}, {'CPOL_GATE1': '0'}
SLOTS = ('QR_v', 'QS_v', 'QG_v')                 # the mass densities of hydrometeor slots 0, 1, 2 of the c2 workload
CUBES = ('all_present', 'all_absent', 'last_slot_only', 'slots_0_and_2', 'one_gate')
COMBOS = tuple((att, rvel) for att in (1, 0) for rvel in (True, False))
N_SWEEPS = 4                                      # on one context: full form, recording, replay, replay


def _fields(rvel):
    import bench
    return tuple(bench.RADAR_FIELDS) + (('RVEL',) if rvel else ()) + ('mask',)


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)                        # (read when the context is created)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _conf(att):
    import bench
    conf = bench.bench_config(True)
    conf['radar'].update(range=RES * N_GATES, radial_resolution=RES)
    conf['microphysics']['with_attenuation'] = att
    return conf


def _rays():
    return np.linspace(3.0, 3.0 + 0.997 * (N_RAYS - 1), N_RAYS), np.full(N_RAYS, 2.0)


def _operator(env, conf, luts, cube, output='only_radar'):
    from cosmo_pol_amd import RadarOperator
    with _env(env):
        op = RadarOperator(config=copy.deepcopy(conf), luts=luts, output_variables=output)
        op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    return op


def _field(shape, level, tilt):
    """A positive mass density without two equal values along any axis (no plateau: a unique largest gate)."""
    nz, ny, nx = shape
    f = (1.0 + tilt[0] * np.arange(nz)[:, None, None] / nz + tilt[1] * np.arange(ny)[None, :, None] / ny
         + tilt[2] * np.arange(nx)[None, None, :] / nx)
    return (level * f).astype(np.float32)


def _cubes(luts):
    """{name: cube}: the small test cube with the three mass densities replaced."""
    import bench
    base = bench.make_inputs('c2', True)[2]
    shape = base['data']['T'].shape
    fields = {'QR_v': _field(shape, 4e-4, (0.3, 0.2, 0.1)), 'QS_v': _field(shape, 3e-4, (-0.2, 0.1, 0.3)),
              'QG_v': _field(shape, 5e-4, (0.5, 0.3, 0.2))}
    zero = np.zeros(shape, dtype=np.float32)

    def cube(present):
        c = dict(base)
        c['data'] = dict(base['data'])
        for k in SLOTS:
            c['data'][k] = fields[k] if k in present else zero
        return c

    out = {'all_present': cube(SLOTS), 'all_absent': cube(()), 'last_slot_only': cube(SLOTS[2:]),
           'slots_0_and_2': cube((SLOTS[0], SLOTS[2]))}
    # one species in ONE gate of ONE ray: the interpolation is linear, so the field minus the mean of its two largest
    # interpolated values is positive at the largest gate alone (a mass density <= 0 is no item)
    probe = _operator(GENERAL, _conf(1), luts, out['last_slot_only'], output='all')
    az, el = _rays()
    q = probe.simulate_rays(az, el, apply_sensitivity=False)['model_vars'][list(probe._staged_vars).index('QG_v')]
    top = np.sort(q[np.isfinite(q)])[-2:]
    assert q.shape == (N_RAYS, N_GATES) and top[1] - top[0] > 1e-4 * top[1], top
    one = cube(())
    one['data']['QG_v'] = (fields['QG_v'] - np.float32(0.5 * (top[0] + top[1]))).astype(np.float32)
    probe.load_model_arrays(one['data'], one['zlevels'], one['proj_info'], one['resolution'])
    q = probe.simulate_rays(az, el, apply_sensitivity=False)['model_vars'][list(probe._staged_vars).index('QG_v')]
    probe.close()
    assert int((q > 0).sum()) == 1, int((q > 0).sum())
    out['one_gate'] = one
    return out


class _Slab(object):
    """The outputs of one sweep in device memory; RVEL only where it is asked for."""

    def __init__(self, rvel):
        import torch
        import bench
        self.rvel = rvel
        self.f32 = torch.full((len(bench.RADAR_FIELDS), N_RAYS, N_GATES), -7.0, dtype=torch.float32, device='cuda')
        self.f64 = torch.full((2, N_RAYS, N_GATES), -7.0, dtype=torch.float64, device='cuda')
        self.ptrs = dict({k: self.f32[i].data_ptr() for i, k in enumerate(bench.RADAR_FIELDS)}, mask=self.f64[1].data_ptr())
        if rvel:
            self.ptrs['RVEL'] = self.f64[0].data_ptr()

    def numpy(self):
        import torch
        import bench
        torch.cuda.synchronize()
        a, b = self.f32.cpu().numpy(), self.f64.cpu().numpy()
        out = dict({k: a[i] for i, k in enumerate(bench.RADAR_FIELDS)}, mask=b[1])
        if self.rvel:
            out['RVEL'] = b[0]
        return out


def _sweep(op, rvel, mode):
    """-> (arrays, stencil form of the sweep); the launch form asserted as tests/test_gpu_gate_tiles.py does"""
    az, el = _rays()
    slab = _Slab(rvel)
    op.simulate_rays(az, el, device_outputs=slab.ptrs, apply_sensitivity=True)
    forms = op._ctx.launch_forms()
    form = op.stencil_state()['form']
    op.wait()
    if mode == 'lanes':
        assert forms['gate1_ray'] == 1 and forms['gate1'] == 1, forms
    else:
        assert forms['gate1'] == 0, forms
    return slab.numpy(), form


def _run(mode, cubes, luts, n_sweeps):
    """{(cube, attenuation, rvel): [arrays per sweep]} and the stencil forms met, one operator per attenuation setting"""
    out, forms = {}, []
    for att in (1, 0):
        op = None
        for name in CUBES:
            c = cubes[name]
            if op is None:
                op = _operator(LANES if mode == 'lanes' else GENERAL, _conf(att), luts, c)
            else:
                op.load_model_arrays(c['data'], c['zlevels'], c['proj_info'], c['resolution'])
            for rvel in (True, False):
                got = [_sweep(op, rvel, mode) for _ in range(n_sweeps)]
                out[(name, att, rvel)] = [g[0] for g in got]
                forms.append([g[1] for g in got])
        op.close()
    return out, forms


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b, rvel, what):
    for k in _fields(rvel):
        assert a[k].shape == b[k].shape == (N_RAYS, N_GATES) and a[k].dtype == b[k].dtype, (what, k)
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, int((_bits(a[k]) != _bits(b[k])).sum()))


@pytest.fixture(scope='module')
def runs():
    import bench
    luts = bench.make_inputs('c2', True)[3]
    cubes = _cubes(luts)
    general, _ = _run('general', cubes, luts, 1)
    lanes, forms = _run('lanes', cubes, luts, N_SWEEPS)
    return {'general': general, 'lanes': lanes, 'forms': forms}


@pytest.mark.parametrize('att,rvel', COMBOS)
@pytest.mark.parametrize('name', CUBES)
def test_lanes_path_has_the_general_sequence_bits(runs, name, att, rvel):
    want = runs['general'][(name, att, rvel)][0]
    for s, got in enumerate(runs['lanes'][(name, att, rvel)]):
        _same_bits(got, want, rvel, (name, att, rvel, s))


def test_the_cubes_put_every_kind_of_tile_in_front_of_the_kernel(runs):
    valid = {name: np.isfinite(runs['general'][(name, 1, True)][0]['ZH']) for name in CUBES}
    inside = runs['general'][('all_present', 1, True)][0]['mask'] == 0
    assert inside.sum() > N_RAYS * N_GATES // 2
    # the sensitivity cut aside (apply_sensitivity takes weak gates), gates with a species hold values, clear air holds NaN
    assert valid['all_present'].sum() > inside.sum() // 2
    assert valid['all_absent'].sum() == 0
    assert valid['last_slot_only'].sum() > inside.sum() // 4 and valid['slots_0_and_2'].sum() > inside.sum() // 4
    assert valid['one_gate'].sum() <= 1
    # the sweeps of one context went through the stencil's life cycle: recording and replay are among the forms, and every
    # case ended replaying
    forms = runs['forms']
    assert forms[0] == [0, 1, 2, 2], forms[0]
    assert all(f[-1] == 2 for f in forms), forms


def test_child_without_presence_words_gives_the_same_bits(runs, tmp_path):
    """CPOL_GATE1_PRESENT is read once per process: a child takes the all-present path (every wavefront a ticket)."""
    import subprocess
    out = str(tmp_path / 'child.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, CPOL_GATE1_PRESENT='0'),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'child ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(out)
    for name in CUBES:
        for att, rvel in COMBOS:
            mine = runs['lanes'][(name, att, rvel)][-1]
            child = {k: got['%s/%d/%d/%s' % (name, att, int(rvel), k)] for k in _fields(rvel)}
            _same_bits(child, mine, rvel, ('child', name, att, rvel))


def _child(path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import bench
    assert os.environ.get('CPOL_GATE1_PRESENT') == '0'
    luts = bench.make_inputs('c2', True)[3]
    res, _ = _run('lanes', _cubes(luts), luts, 1)
    np.savez(path, **{'%s/%d/%d/%s' % (name, att, int(rvel), k): v[0][k] for (name, att, rvel), v in res.items() for k in v[0]})
    print('child ok')


if __name__ == '__main__':
    _child(sys.argv[1])
