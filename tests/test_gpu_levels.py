"""The level search of the gate kernel (gate_geometry, cosmo_pol_amd/csrc/cpol_interp.inl) at every level count at which it
takes another path: the bisection (nz = 3, nz > 144), the wide count over every 16th level and four clamped windows (nz = 4 ..
81) and the same with the second group of sixteenths (nz = 82 .. 144), with neighbour columns tens of levels apart and heights
exactly on levels, column tops and the blended topography (tests/_levels.py).

  a. cpol_interp_points against the NumPy restatement on all points (the domain's upper edge included, where the clamp of
     the restatement is the definition) and against the oracle's C twin on the interior ones;
  b. the staging kernels at 1, 3 and CPOL_MAX_VARS variables: every variable's values, and the staged arrays as they lie in
     device memory;
  c. the sweep forms on two radial cases with roughened cubes at seven level counts: cpol_interp_subbeams against the oracle,
     the round trip through columns, an ensemble through k_interp_members.
Everything is bit equality; no tolerance is introduced.

Tried against scratch builds with one edit each (comparisons only, every address as before): without the second group of
sixteenths (`if (false && nz - 2 >= 16 * 5)`) the point tests fail at nz = 97 .. 144 and the sweeps at 98 and 144 (at nz = 82
and 83 the windows behind the fourth sixteenth still reach level 80, and an index of nz - 2 gives the values of nz - 3: the
same bits); `>` for `>=` in the window count fails at every nz = 4 .. 144, in the neighbour walk at every nz from 4 (at nz = 3
the values do not depend on the index).  `>` for `>=` in the count of sixteenths is the same search -- the window tests that
level again -- and so is the bisection alone (CPOL_LEVEL_SEARCH_WIDE=0): both pass, as they must."""
import numpy as np
import pytest

import _cases
import _levels as L
from cosmo_pol_oracle import beam

pytestmark = pytest.mark.gpu

FORMS_SEEN = {}                                  # (case, nz) -> launch_forms() of simulate_rays


@pytest.fixture(scope='module')
def ctx():
    from cosmo_pol_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def operators():
    """One operator per radial case for the whole module, restaged per level count.  The single-beam case melts: its operator
    is created with CPOL_GATE1=2 (read when the context is created), so that its sweeps take k_interp_sweep and the single-beam
    gate kernel; the 7 x 7 case takes k_interp_classify."""
    from cosmo_pol_amd import RadarOperator
    ops = {}
    with pytest.MonkeyPatch.context() as mp:
        for k in ('CPOL_GATE1', 'CPOL_FUSE_GATE1', 'CPOL_FUSE_CLASSIFY', 'CPOL_RARE_DIRECT', 'CPOL_GATE1_RAY', 'CPOL_GATE1_SPECIES'):
            mp.delenv(k, raising=False)
        for name in L.SWEEP_CASES:
            if name == 'c3_melt_ice':
                mp.setenv('CPOL_GATE1', '2')
            else:
                mp.delenv('CPOL_GATE1', raising=False)
            case = L.sweep_case(name, L.NZ_SWEEP[0])
            ops[name] = RadarOperator(config=case['over'], luts=case['luts'], output_variables='only_radar')
    yield ops
    for op in ops.values():
        op.close()


def _assert_points(got, ref, c, sel, tag):
    assert got.dtype == np.float32
    want = {k: v[..., sel] if k == 'values' else v[sel] for k, v in ref.items()}
    assert L.same_bits(got[sel], want['values']), \
        '%s: %s' % (tag, L.first_differences(got[sel], want, c['heights'][sel], c['coords'][sel]))


# ---------------------------------------------------------------- a. points, every level count

@pytest.mark.parametrize('nz', L.NZ_POINTS)
def test_points_at_every_level_count(ctx, nz):
    c = L.case(nz)
    assert not L.coverage_failures(nz, c['ref'])
    T, zl = c['cube']['data']['T'], c['cube']['zlevels']
    ctx.stage_model([T, c['second']], zl, c['llc'], c['urc'], c['res'], L.SOUTH_POLE)
    out = ctx.interp_points(c['coords'], c['heights'])
    assert out.shape == (2, c['heights'].size)
    everything = np.ones(c['heights'].size, dtype=bool)
    for v, (ref, data) in enumerate(((c['ref'], T), (c['ref2'], c['second']))):
        _assert_points(out[v], ref, c, everything, 'nz %d variable %d against the restatement' % (nz, v))
        inside = c['interior']
        twin = beam.get_all_radar_pts(c['coords'][inside], c['heights'][inside], data, zl, c['llc'], c['res'])
        assert L.same_bits(out[v][inside], twin), 'nz %d variable %d against the C twin' % (nz, v)


# ---------------------------------------------------------------- b. variable counts of the staging kernels

@pytest.mark.parametrize('n_vars', [1, 3, 24])
def test_staging_at_other_variable_counts(ctx, n_vars):
    from cosmo_pol_amd import _native
    assert _native.CPOL_MAX_VARS == 24
    nz = 82
    c = L.case(nz)
    zl = c['cube']['zlevels']
    _, ny, nx = zl.shape
    rng = np.random.default_rng(n_vars)
    cubes = np.stack([c['cube']['data']['T']] + [rng.normal(size=zl.shape).astype(np.float32) for _ in range(n_vars - 1)])
    ctx.stage_model(list(cubes), zl, c['llc'], c['urc'], c['res'], L.SOUTH_POLE)
    out = ctx.interp_points(c['coords'], c['heights'])
    assert out.shape == (n_vars, c['heights'].size)
    ref = L.reference_points(cubes, zl, c['llc'], c['res'], c['coords'], c['heights'])
    assert L.same_bits(ref['values'][0], c['ref']['values'])
    for v in range(n_vars):
        one = dict(ref, values=ref['values'][v])
        _assert_points(out[v], one, c, np.ones(c['heights'].size, dtype=bool), '%d variables, variable %d' % (n_vars, v))
    # the staged model as it lies in device memory: [ny][nx][nz][n_vars], [ny][nx][nz], [ny][nx](top, lowest level)
    assert np.array_equal(ctx.debug_read('model_v', (ny, nx, nz, n_vars), np.float32).view(np.uint32),
                          np.ascontiguousarray(cubes.transpose(2, 3, 1, 0)).view(np.uint32))
    assert np.array_equal(ctx.debug_read('model_h', (ny, nx, nz), np.float32), zl.transpose(1, 2, 0))
    assert np.array_equal(ctx.debug_read('model_ht', (ny, nx, 2), np.float32), np.stack([zl[0], zl[nz - 1]], axis=-1))


# ---------------------------------------------------------------- c. the sweep forms

def _load(op, cube):
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])


def _equal_results(got, ref, tag):
    assert set(ref) == set(got), (tag, set(ref) ^ set(got))
    n = 0
    for k, v in ref.items():
        if not isinstance(v, np.ndarray):
            assert got[k] == v, (tag, k)
            continue
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, (tag, k)
        assert np.array_equal(got[k], v, equal_nan=True), (tag, k)
        n += 1
    assert n >= 10, (tag, n)                     # the polarimetric fields and the mask at least


@pytest.mark.parametrize('nz', L.NZ_SWEEP)
@pytest.mark.parametrize('name', L.SWEEP_CASES)
def test_sweep_forms_on_rough_cubes(operators, name, nz):
    case = L.sweep_case(name, nz)
    # coverage, from the oracle's sub-radials alone
    assert not L.sweep_coverage_failures(nz, case), L.sweep_coverage_failures(nz, case)
    op = operators[name]
    _load(op, case['cube'])
    az = np.array([r[0] for r in case['rays']])
    el = np.array([r[1] for r in case['rays']])
    # cpol_interp_subbeams against the oracle, ray by ray
    for (a, e), subs in zip(case['rays'], case['subs']):
        _cases.assert_radial_equals_oracle(op.get_interpolated_radial(a, e), subs)
    # the sweep, and the round trip through the columns
    ref = op.simulate_rays(az, el, apply_sensitivity=False)
    forms = op._ctx.launch_forms()
    FORMS_SEEN[(name, nz)] = forms
    assert np.isfinite(ref['ZH']).sum() > 10
    for melting in (True, False):
        cols = op.interpolate_rays(az, el, melting=melting)
        assert ('QmS_v' in cols) == melting
        got = op.simulate_columns(cols)
        assert op._ctx.launch_forms()['interp_classify'] == 0
        _equal_results(got, ref, '%s nz %d melting %s' % (name, nz, melting))


@pytest.mark.parametrize('nz', [82, 145])
def test_ensemble_shares_the_geometry(operators, nz):
    """k_interp_members: a two-member ensemble on the 7 x 7 case, the shared-geometry sweep against member by member."""
    name = 'c4_7x7'
    case = L.sweep_case(name, nz)
    op = operators[name]
    cube = case['cube']
    other = dict(cube['data'])
    other['T'] = (cube['data']['T'] + np.float32(0.5)).astype(np.float32)
    other['QR_v'] = (cube['data']['QR_v'] * np.float32(1.1)).astype(np.float32)
    op.load_model_ensemble([cube['data'], other], cube['zlevels'], cube['proj_info'], cube['resolution'])
    assert op.n_members == 2
    az = np.array([r[0] for r in case['rays']])
    el = np.array([r[1] for r in case['rays']])
    shared = op.simulate_rays_ensemble(az, el, form='shared', apply_sensitivity=False)
    forms = op._ctx.launch_forms()
    assert forms['interp_classify'] == 0 and forms['n_sub'] == 49, forms
    each = op.simulate_rays_ensemble(az, el, form='per_member', apply_sensitivity=False)
    _equal_results(shared, each, 'ensemble nz %d' % nz)
    zh = shared['ZH']
    assert np.isfinite(zh[0]).sum() > 10
    assert (~((zh[0] == zh[1]) | (np.isnan(zh[0]) & np.isnan(zh[1])))).sum() > 0
    _load(op, cube)                              # (the members go)
    assert op.n_members == 1


def test_launch_forms_reached_the_second_group(operators):
    """Both kernels that carry gate_geometry through a sweep ran where the second group of sixteenths runs (nz >= 82): the
    single-beam gate kernel behind k_interp_sweep, and k_interp_classify."""
    for name in L.SWEEP_CASES:
        if not any(k == (name, nz) for k in FORMS_SEEN for nz in L.NZ_SWEEP if nz >= 82):      # (run alone: sweep now)
            case = L.sweep_case(name, 82)
            _load(operators[name], case['cube'])
            operators[name].simulate_rays([case['rays'][0][0]], [case['rays'][0][1]], apply_sensitivity=False)
            FORMS_SEEN[(name, 82)] = operators[name]._ctx.launch_forms()
    print({k: (v['gate1'], v['interp_classify'], v['n_sub']) for k, v in sorted(FORMS_SEEN.items())})
    high = [v for (name, nz), v in FORMS_SEEN.items() if nz >= 82]
    assert any(v['gate1'] == 1 and v['n_sub'] == 1 for v in high), 'the single-beam gate kernel never ran at nz >= 82'
    assert any(v['interp_classify'] == 1 for v in high), 'k_interp_classify never ran at nz >= 82'
