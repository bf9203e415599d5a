"""Neighbourhood verification on the GPU through the sweeps (cpol_outputs.fractions beside cpol_outputs.composite): the scores of
a call against neighbourhood.sums of the maps THE SAME CALL returns, np.array_equal on uint64, and those maps against
composite.compose / composite.finish as before.  The observed map is the composite of the case's second cube (another state of
the same model), the thresholds are values of the forecast map itself, and the rule is asserted to give 0 < FSS < 1 somewhere, so
no test passes on empty or identical maps.

Cases: the golden radials c2_rsg (single beam) and c5_2mom_dop2_sub (Doppler scheme 2), seven rays at az + 0.5 k."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_ensemble as E
from test_gpu_composite_sweeps import assert_maps, maps_of, plain_run, rule, same, same_gates, spec_for
from test_gpu_histogram_sweeps import arrays, op_for, rays, _ops

pytestmark = pytest.mark.gpu

NAMES = ['c2_rsg', 'c5_2mom_dop2_sub']
f4, u1, u8 = np.float32, np.uint8, np.uint64
KEYS = ('diff2', 'forecast2', 'observed2', 'n_forecast', 'n_observed', 'n_domain')
RADII = [0, 1, 2, 5]


def NB():
    from cosmo_pol_amd import neighbourhood
    return neighbourhood


@pytest.fixture(scope='module', autouse=True)
def _close_operators():
    yield
    for op in _ops.values():
        op.close()
    _ops.clear()


def values_of(m, qs=(0.2, 0.4, 0.6, 0.8)):
    """Thresholds that ARE values of the map `m`: its finite values at the given ranks."""
    v = np.sort(np.asarray(m, dtype=np.float64)[np.isfinite(m)])
    assert v.size >= 8, v.size
    return [float(v[int(q * (v.size - 1))]) for q in qs]


@functools.lru_cache(maxsize=None)
def setup(name):
    """(operator on cube 0, az, el, the composite's spec, the Fractions of ZH 'max', the observed map: the composite of cube 1,
    a partial domain)"""
    op = op_for(name, 0)
    az, el = rays(name)
    cspec = spec_for(plain_run(name, 0)[0], az, products=('max', 'lowest'), slab=False, fields=['ZH', 'KDP'], n=(23, 17))
    forecast = np.array(op.simulate_rays_composite(az, el, cspec)['composite']['values']['ZH']['max'][0])
    observed = np.array(op_for(name, 1).simulate_rays_composite(az, el, cspec)['composite']['values']['ZH']['max'][0])
    assert observed.dtype == f4 and observed.shape == (cspec.n_y, cspec.n_x) and not same(observed, forecast)
    spec = NB().Fractions(cspec, 'ZH', values_of(forecast), RADII)
    domain = np.ones(observed.shape, u1)
    domain[:, :2] = 0
    domain[-1] = 0
    return op, az, el, cspec, spec, observed, domain


def assert_scores(got, want, tag, skilful=False):
    for k in KEYS:
        assert got[k].dtype == u8 and np.array_equal(np.array(got[k]), want[k]), (tag, k, np.array(got[k]).ravel()[:8], want[k].ravel()[:8])
    assert np.array_equal(got['radii'], want['radii']) and np.array_equal(got['thresholds'], want['thresholds']), tag
    assert want['forecast2'].any() and want['observed2'].any(), (tag, 'the rule counts nothing')
    score = NB().fss(want)
    print('%s: FSS %s' % (tag, np.array2string(score, precision=3)))
    if skilful:
        assert ((score > 0.0) & (score < 1.0)).any(), (tag, score)


def scored(res, spec, observed, domain, tag, plane='max', skilful=False):
    """The scores of `res` against the rule applied to the maps `res` itself carries."""
    maps = maps_of(res)
    want = NB().sums(spec, maps['values'][spec.field][plane], observed, domain)
    assert_scores(res['composite']['fractions'], want, tag, skilful)
    return maps, want


# ---------------------------------------------------------------------------------------------------- scores equal the rule
@pytest.mark.parametrize('name', NAMES)
def test_scores_equal_the_rule(name):
    op, az, el, cspec, spec, observed, domain = setup(name)
    res = op.simulate_rays_composite_fss(az, el, spec, observed, keep_gates=True)
    maps, want = scored(res, spec, observed, None, name, skilful=True)
    assert_maps(maps, rule(cspec, [(arrays(res), az)]), cspec, name)                # the maps are the composite's, as before
    assert want['n_domain'].shape == (1, 4) and (want['n_domain'] == cspec.n_x * cspec.n_y).all()
    with_domain = op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain)
    assert 'ZH' not in with_domain
    _, wd = scored(with_domain, spec, observed, domain, name + '/domain', skilful=True)
    assert (wd['n_domain'] == int(domain.sum())).all() and not np.array_equal(wd['forecast2'], want['forecast2'])
    # a bool domain is the same domain; another field and plane, thresholds in that plane's units; a block per ray
    as_bool = op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain.astype(bool))
    assert_scores(as_bool['composite']['fractions'], wd, name + '/bool domain')
    low = NB().Fractions(cspec, 'KDP', values_of(maps['values']['KDP']['height_of_lowest'][0], (0.3, 0.7)), [0, 3], plane='height_of_lowest')
    obs_low = np.roll(maps['values']['KDP']['height_of_lowest'][0], 1, axis=1)
    scored(op.simulate_rays_composite_fss(az, el, low, obs_low), low, obs_low, None, name + '/KDP height_of_lowest',
           plane='height_of_lowest')
    per_ray = op.simulate_rays_composite_fss(az, el, spec, observed, rays_per_block=1)
    _, wr = scored(per_ray, spec, observed, None, name + '/per ray')
    assert wr['diff2'].shape == (len(az), 4, len(RADII)) and (wr['n_forecast'].sum(axis=0) >= want['n_forecast'][0]).all()


# ---------------------------------------------------------------------------------------------------- output modes
def captured(op, call):
    """call(), and copies of the cpol_sweep_params / cpol_ray_tables_t it handed to Context.run_sweep"""
    from cosmo_pol_amd import _native as N
    ctx, seen = op._ctx, {}
    orig = ctx.run_sweep

    def spy(p, t, o):
        seen['p'], seen['t'] = N.SweepParams.from_buffer_copy(p), N.RayTables.from_buffer_copy(t)
        seen['slots'] = (bool(o.composite), bool(o.fractions))
        return orig(p, t, o)
    ctx.run_sweep = spy
    try:
        res = call()
    finally:
        del ctx.run_sweep
    return res, seen


def direct(op, spec, az, p, t, observed, domain=None, phase=3, change=None, comp_change=None, outputs=None, entry='run_sweep'):
    """One blocking cpol_run_sweep (outputs_on_device 0) with a cpol_composite and a cpol_fractions of its own, plain host arrays
    -> (maps, scores)."""
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import composite as CP
    cspec = spec.composite
    c, keep = N.Context.composite_struct(cspec, phase=phase, azimuths=az)
    vals = {k: np.full((1, len(cspec.planes(k)), cspec.n_y, cspec.n_x), 77.0, f4) for k in cspec.fields}
    cnt = np.full((1, len(cspec.fields), cspec.n_y, cspec.n_x), 77, u8)
    for k in cspec.fields:
        c.values[CP.FIELDS.index(k)] = vals[k].ctypes.data
    c.count = cnt.ctypes.data
    f, _ = N.Context.fractions_struct(spec)
    s = np.full((1, len(spec.thresholds), len(spec.radii), 3), 77, u8)
    tt = np.full((1, len(spec.thresholds), 3), 77, u8)
    obs = np.ascontiguousarray(observed)
    f.observed, f.sums, f.totals = obs.ctypes.data, s.ctypes.data, tt.ctypes.data
    if domain is not None:
        dom = np.ascontiguousarray(domain)
        f.domain = dom.ctypes.data
    if comp_change:
        keep.append(comp_change(c))
    if change:
        keep.append(change(f))
    o = N.Outputs()
    o.composite, o.fractions = C.pointer(c), C.pointer(f)
    if outputs:
        keep.append(outputs(o))
    q = N.SweepParams.from_buffer_copy(p)
    q.outputs_on_device = 0
    if entry == 'run_columns':
        op._ctx.run_columns(q, N.Columns(), o)
    else:
        op._ctx.run_sweep(q, t, o)
    op.wait()
    del keep
    maps = {'values': {k: {p_: vals[k][:, j] for j, p_ in enumerate(cspec.planes(k))} for k in cspec.fields},
            'count': {k: cnt[:, i] for i, k in enumerate(cspec.fields)}}
    return maps, NB().result(spec, s, tt)


@pytest.mark.parametrize('name', NAMES)
def test_output_modes(name):
    """Page-locked buffers (waited for, and pinned=True + wait), blocking host buffers and device pointers carry the same scores."""
    import torch
    op, az, el, cspec, spec, observed, domain = setup(name)
    locked, seen = captured(op, lambda: op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain))
    assert seen['slots'] == (True, True)
    good, want = scored(locked, spec, observed, domain, name + '/page-locked', skilful=True)
    lazy = op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain, pinned=True)
    op.wait()
    assert_maps(maps_of(lazy), good, cspec, name + '/pinned')
    assert_scores(lazy['composite']['fractions'], want, name + '/pinned')
    maps, got = direct(op, spec, az, seen['p'], seen['t'], observed, domain)
    assert_maps(maps, good, cspec, name + '/blocking')
    assert_scores(got, want, name + '/blocking')
    _, got = direct(op, spec, az, seen['p'], seen['t'], observed)             # (NULL domain: every cell)
    assert_scores(got, NB().sums(spec, good['values']['ZH']['max'], observed), name + '/blocking, no domain')
    # device outputs: the maps, the observed map, the domain and the scores are device pointers; a pass of two calls writes
    # nothing before its finish
    dv = {k: torch.full((1, len(cspec.planes(k)), cspec.n_y, cspec.n_x), 77.0, dtype=torch.float32, device='cuda') for k in cspec.fields}
    dc = torch.full((1, len(cspec.fields), cspec.n_y, cspec.n_x), 77, dtype=torch.int64, device='cuda')
    ds = torch.full((1, len(spec.thresholds), len(RADII), 3), 77, dtype=torch.int64, device='cuda')
    dt = torch.full((1, len(spec.thresholds), 3), 77, dtype=torch.int64, device='cuda')
    d_obs, d_dom = torch.from_numpy(observed).cuda(), torch.from_numpy(domain).cuda()
    entry = {'values': {k: a.data_ptr() for k, a in dv.items()}, 'count': dc.data_ptr(), 'observed': d_obs.data_ptr(),
             'domain': d_dom.data_ptr(), 'sums': ds.data_ptr(), 'totals': dt.data_ptr()}
    op.simulate_rays_composite_fss(az, el, spec, None, phase=1, device_outputs={'composite': entry})
    op.wait()
    assert (ds == 77).all().item() and (dt == 77).all().item() and (dc == 77).all().item()
    op.simulate_rays_composite_fss(az, el, spec, None, phase=2, device_outputs={'composite': entry})
    op.wait()
    # (the same sweep folded twice: maxima and minima are those of one, so the plane and its scores are, too)
    assert same(dv['ZH'].cpu().numpy()[:, 0], good['values']['ZH']['max'])
    assert_scores(NB().result(spec, ds.cpu().numpy().view(u8), dt.cpu().numpy().view(u8)), want, name + '/device')
    with pytest.raises(ValueError, match='not both'):
        op.simulate_rays_composite_fss(az, el, spec, observed, device_outputs={'composite': entry})
    with pytest.raises(ValueError, match='observed'):
        op.simulate_rays_composite_fss(az, el, spec, None)


# ---------------------------------------------------------------------------------------------------- passes
def test_three_call_pass():
    """A pass cut into three calls is scored only at its end and equals the pass in one call."""
    name = 'c2_rsg'
    op, az, el, cspec, spec, observed, domain = setup(name)
    whole = op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain)
    good, want = scored(whole, spec, observed, domain, 'one call', skilful=True)
    parts = []
    for rows, phase in ((slice(0, 3), 1), (slice(3, 5), 0), (slice(5, 7), 2)):
        res, seen = captured(op, lambda: op.simulate_rays_composite_fss(az[rows], el[rows], spec, observed, domain=domain, phase=phase))
        assert seen['slots'] == (True, phase == 2)                # (the struct goes with the finishing call alone)
        parts.append(res)
    assert 'composite' not in parts[0] and 'composite' not in parts[1]
    assert_maps(maps_of(parts[2]), good, cspec, 'three calls')
    assert_scores(parts[2]['composite']['fractions'], want, 'three calls')


def test_scans():
    """get_PPI_composite_fss: the volume folds in one pass and is scored once, at its end; per_sweep gives a list."""
    name = 'c2_rsg'
    op = op_for(name, 0, lanes=2)
    _, az, _, cspec, spec, observed, domain = setup(name)
    elevations = [4.0, 5.0, 6.0]
    volume = op.get_PPI_composite_fss(elevations, spec, observed, domain=domain, azimuths=az, keep_gates=True)
    assert len(volume['sweeps']) == 3 and all('composite' not in s for s in volume['sweeps'])
    maps, _ = scored(volume, spec, observed, domain, 'volume')
    assert_maps(maps, rule(cspec, [(arrays(s), az) for s in volume['sweeps']]), cspec, 'volume')
    assert_maps(maps_of(op.get_PPI_composite(elevations, cspec, azimuths=az)), maps, cspec, 'volume without scores')
    per_sweep = op.get_PPI_composite_fss(elevations, spec, observed, azimuths=az, per_sweep=True)
    assert len(per_sweep) == 3
    wants = [scored(per_sweep[i], spec, observed, None, 'sweep %d' % i)[1] for i in range(3)]
    assert not np.array_equal(wants[0]['diff2'], wants[2]['diff2'])


def test_time_blend():
    import test_gpu_timed as T
    name = 'c2_rsg'
    op, _, _ = T.series_operator(name)
    _, az, el, cspec, spec, observed, domain = setup(name)
    res = op.simulate_rays_at_composite_fss(az, el, 200.0, spec, observed, domain=domain, keep_gates=True)
    maps, _ = scored(res, spec, observed, domain, 'timed')
    assert_maps(maps, rule(cspec, [(arrays(res), az)]), cspec, 'timed')
    assert_maps(maps_of(op.simulate_rays_at_composite(az, el, 200.0, cspec)), maps, cspec, 'timed without scores')
    op.close()


def test_ensemble():
    """One row of scores per member, equal to the member's own call, with the member list in one chunk and in one per member."""
    name = 'c2_rsg'
    op, _, _ = E.ensemble_operator(name)
    _, az, el, cspec, spec, observed, domain = setup(name)
    got = op.simulate_rays_ensemble_composite_fss(az, el, spec, observed, domain=domain)
    maps, want = scored(got, spec, observed, domain, 'ensemble', skilful=True)
    assert want['diff2'].shape == (3, 4, len(RADII)) and not np.array_equal(want['diff2'][0], want['diff2'][1])
    assert_maps(maps_of(op.simulate_rays_ensemble_composite(az, el, cspec)), maps, cspec, 'ensemble without scores')
    for m in range(3):
        op.select_member(m)
        alone = op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain)['composite']['fractions']
        for k in KEYS:
            assert np.array_equal(np.array(alone[k]), want[k][m:m + 1]), (m, k)
    op.select_member(0)
    op.sequence_memory_budget = 1
    cut = op.simulate_rays_ensemble_composite_fss(az, el, spec, observed, domain=domain)
    cut_whole = op.simulate_rays_ensemble_composite_fss(az, el, spec, observed, domain=domain, per_member=False)
    op.sequence_memory_budget = None
    assert_maps(maps_of(cut), maps, cspec, 'ensemble in chunks')
    assert_scores(cut['composite']['fractions'], want, 'ensemble in chunks')
    whole = op.simulate_rays_ensemble_composite_fss(az, el, spec, observed, domain=domain, per_member=False)
    _, ww = scored(whole, spec, observed, domain, 'ensemble, one map')
    assert ww['diff2'].shape == (1, 4, len(RADII))
    assert_scores(cut_whole['composite']['fractions'], ww, 'ensemble in chunks, one map')
    op.close()


# ---------------------------------------------------------------------------------------------------- composites are left alone
def test_composites_stencils_and_forms_are_left_alone():
    """Five sweeps of one geometry with the scores and five without: the same maps and per-gate arrays bit for bit, the same
    stencil forms (full, recording, replay ...) and launch forms sweep by sweep."""
    from test_gpu_ensemble import case, load, operator
    name = 'c2_rsg'
    conf, luts, cubes, _, _ = case(name)
    _, az, el, cspec, spec, observed, domain = setup(name)
    seen = {}
    for with_scores in (False, True):
        op = operator(conf, luts)
        load(op, cubes[0])
        st, forms, out = [], [], []
        for i in range(5):
            res = (op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain, keep_gates=True) if with_scores
                   else op.simulate_rays_composite(az, el, cspec, keep_gates=True))
            out.append((arrays(res), maps_of(res)))
            assert ('fractions' in res['composite']) == with_scores
            st.append(op.stencil_state()['form'])
            forms.append(op._ctx.launch_forms())
        if with_scores:                       # ... and a composite call behind scored ones returns what it returned before
            after = op.simulate_rays_composite(az, el, cspec, keep_gates=True)
            assert 'fractions' not in after['composite']
            assert_maps(maps_of(after), seen[False][2][0][1], cspec, 'a composite call behind scored ones')
        seen[with_scores] = (st, forms, out)
        op.close()
    print('stencil forms without / with the scores:', seen[False][0], seen[True][0])
    assert seen[False][0] == seen[True][0] and seen[True][0][-1] == 2
    assert seen[False][1] == seen[True][1]
    for i in range(5):
        for k, v in seen[False][2][i][0].items():
            assert same_gates(seen[True][2][i][0][k], v), (i, k)
        assert_maps(seen[True][2][i][1], seen[False][2][i][1], cspec, 'sweep %d' % i)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_pass_and_the_context_usable():
    name = 'c2_rsg'
    op, az, el, cspec, spec, observed, domain = setup(name)
    whole, seen = captured(op, lambda: op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain))
    good, want = scored(whole, spec, observed, domain, 'before the refusals')
    p, t = seen['p'], seen['t']
    # a pass is open while the refusals come
    op.simulate_rays_composite(az, el, cspec, phase=1)
    op.wait()

    def call(change=None, phase=2, **kw):
        return direct(op, spec, az, p, t, observed, domain, phase=phase, change=change, **kw)

    def item(name_, j, v):
        return lambda f: getattr(f, name_).__setitem__(j, v)
    zv = 1
    assert 'ZV' not in cspec.fields
    for word, change in (('field is not among', lambda f: setattr(f, 'field', zv)), ('field is not among', lambda f: setattr(f, 'field', -1)),
                         ('field is not among', lambda f: setattr(f, 'field', 9)), ('plane lies outside', lambda f: setattr(f, 'plane', 4)),
                         ('plane lies outside', lambda f: setattr(f, 'plane', -1)), ('n_thresholds', lambda f: setattr(f, 'n_thresholds', 0)),
                         ('n_thresholds', lambda f: setattr(f, 'n_thresholds', 5)), ('NaN', item('thresholds', 1, np.nan)),
                         ('n_radii', lambda f: setattr(f, 'n_radii', 0)), ('n_radii', lambda f: setattr(f, 'n_radii', 9)),
                         ('radius must lie', item('radii', 0, -1)), ('radius must lie', item('radii', 3, 1024)),
                         ('ascending', item('radii', 1, 0)), ('ascending', item('radii', 2, 7)),
                         ('observed is NULL', lambda f: setattr(f, 'observed', None)), ('sums or totals', lambda f: setattr(f, 'sums', None)),
                         ('sums or totals', lambda f: setattr(f, 'totals', None))):
        with pytest.raises(ValueError, match=word):
            call(change)
    with pytest.raises(ValueError, match='needs a composite'):
        call(outputs=lambda o: setattr(o, 'composite', None))
    with pytest.raises(ValueError, match='does not finish'):
        call(phase=0)
    with pytest.raises(ValueError, match='does not finish'):
        call(phase=1)
    with pytest.raises(ValueError, match='cpol_composite'):              # (the composite's own refusals come first)
        call(comp_change=lambda c: setattr(c, 'products', 0))
    with pytest.raises(ValueError, match='fractions'):
        call(entry='run_columns', outputs=lambda o: setattr(o, 'composite', None))
    # nothing was queued and the pass is as it was: it finishes with the bits of one sweep folded twice, and is scored
    maps, got = call()
    for k in cspec.fields:
        assert np.array_equal(maps['count'][k], 2 * good['count'][k]), k
        for q in cspec.planes(k):
            assert same(maps['values'][k][q], good['values'][k][q]), (k, q)
    assert_scores(got, want, 'the open pass, finished after the refusals')
    with pytest.raises(ValueError, match='no pass open'):
        call(phase=2)
    maps, got = call(phase=3)
    assert_maps(maps, good, cspec, 'after the refusals')
    assert_scores(got, want, 'after the refusals')
    # the operator's own refusals
    NBm = NB()
    for bad_obs, bad_dom in ((observed.astype(np.float64), None), (observed[:-1], None), (observed.T, None), (observed, domain.astype(np.int32)),
                             (observed, domain[:, :-1])):
        with pytest.raises(ValueError):
            op.simulate_rays_composite_fss(az, el, spec, bad_obs, domain=bad_dom)
    with pytest.raises(ValueError, match='neighbourhood.Fractions'):
        op.simulate_rays_composite_fss(az, el, cspec, observed)
    with pytest.raises(ValueError):
        op.simulate_rays_composite_fss(az, el, spec, observed, rays_per_block=3)
    with pytest.raises(ValueError):
        NBm.Fractions(cspec, 'ZH', [1.0], [2, 1])
    op.distributed = True
    try:
        with pytest.raises(NotImplementedError):
            op.simulate_rays_composite_fss(az, el, spec, observed)
    finally:
        op.distributed = False
    _, last = scored(op.simulate_rays_composite_fss(az, el, spec, observed, domain=domain), spec, observed, domain, 'after the operator refusals')
    for k in KEYS:
        assert np.array_equal(last[k], want[k]), k
