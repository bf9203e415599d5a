"""The NumPy restatement of the gate kernel (tests/_levels.py) against the oracle's C twin, bit for bit, at every level count
tests/test_gpu_levels.py stages -- and the coverage each cube's points must reach for that comparison to pin the level search:
every index, every status, the extrapolation below a lowest level, neighbour columns many levels apart."""
import numpy as np
import pytest

import _levels
from cosmo_pol_oracle import beam


@pytest.fixture(scope='module', params=_levels.NZ_POINTS)
def nz(request):
    """(module scope: both tests of one level count run back to back on one computed case)"""
    return request.param


def test_restatement_equals_the_c_twin(nz):
    c = _levels.case(nz)
    inside = c['interior']
    assert inside.sum() > 0.8 * inside.size
    for ref, data in ((c['ref'], c['cube']['data']['T']), (c['ref2'], c['second'])):
        twin = beam.get_all_radar_pts(c['coords'][inside], c['heights'][inside], data, c['cube']['zlevels'], c['llc'], c['res'])
        want = {k: v[inside] for k, v in ref.items()}
        assert _levels.same_bits(twin, want['values']), \
            _levels.first_differences(twin, want, c['heights'][inside], c['coords'][inside])


def test_points_cover_the_level_search(nz):
    c = _levels.case(nz)
    ref = c['ref']
    ok = ref['status'] == 0
    d = ref['index'][ok, 1:] - ref['index'][ok, :1]
    print('nz %d: %d points, %.2f with a value, neighbour columns %+d .. %+d levels from column 0'
          % (nz, ok.size, ok.mean(), d.min(), d.max()))
    assert c['heights'].size <= 260000
    assert not _levels.coverage_failures(nz, ref), _levels.coverage_failures(nz, ref)


def test_rough_cube_recipe():
    """The cube is make_cube's with only its z-levels rebuilt: the checkerboard and the three model tops are there."""
    cube = _levels.rough_cube(19, seed=5)
    z = cube['zlevels']
    assert z.shape == (19, _levels.NY, _levels.NX) and z.dtype == np.float32
    low = z[-1]
    assert np.abs(low[:-1, :] - low[1:, :]).min() > 2000.0 and np.abs(low[:, :-1] - low[:, 1:]).min() > 2000.0
    # z = topo2 + (top - topo2) eta at the highest and the lowest level, solved for the column's top
    e0, e1 = (18.5 / 19) ** 1.5, (0.5 / 19) ** 1.5
    top = (z[0].astype(np.float64) * (1 - e1) - low.astype(np.float64) * (1 - e0)) / (e0 - e1)
    ii, jj = np.meshgrid(np.arange(_levels.NY), np.arange(_levels.NX), indexing='ij')
    assert np.allclose(top, _levels.TOPS[(ii + 2 * jj) % 3], rtol=0, atol=1.0)
    plain = _levels.synthetic.make_cube(nz=19, ny=_levels.NY, nx=_levels.NX, res=_levels.RES, llc=_levels.LLC, seed=5)
    for k, v in plain['data'].items():
        assert np.array_equal(cube['data'][k], v, equal_nan=True), k


@pytest.mark.parametrize('levels', _levels.NZ_SWEEP)
@pytest.mark.parametrize('name', _levels.SWEEP_CASES)
def test_sweep_rays_cover_the_level_search(name, levels):
    nz = levels
    """The rays tests/test_gpu_levels.py sweeps, from the oracle alone: the gates reach every block of 16 levels and every mask."""
    case = _levels.sweep_case(name, nz)
    print(name, nz, sorted(case['blocks']), sorted(case['masks']), len(case['subs'][0]), len(case['subs'][0][0].mask))
    assert not _levels.sweep_coverage_failures(nz, case), _levels.sweep_coverage_failures(nz, case)
