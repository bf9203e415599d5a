"""Hydrometeor contributions through the sweep (cpol_outputs.species, simulate_rays_species / simulate_rays_at_species), on the
small cubes and operator helpers of tests/test_gpu_ensemble.py: 3 rays x 70 gates; rain alone, R+S+G and R,S,G,mS,mG,I; one
sub-beam (the single-beam fast path would have taken the sweep), three (k_final evaluates in place) and 3 x 3 (k_subbeam_sum);
the sensitivity cut on, attenuation on and off, one case with Doppler scheme 3, one time-blended call.  Per case, BIT FOR BIT:
  (a) every ordinary array of the species call == the plain call's
  (b) res['species']['sz'] == debug_read('sz_integ') of the same sweep in a debug context
  (c) every species array == species.fields_of(sz, ZH, ...) of the call's own sz and ZH
  (d) rain alone, attenuation off: the species' eight fields == the totals'
  (e) launch_forms of the species call: the general sequence; of the plain call behind it: what a fresh operator's plain call takes
No case passes vacuously: a minimum of finite species values, two distinct dominant species where two are present, a censored
gate.  In the R+S+G cubes rain is scaled to a hundredth (RAIN): with the committed cubes rain dominates every gate of these rays,
with it snow takes a third to a half of them.  The constant sensitivity of each case comes from the CPU oracle's ZH along these
rays (70 gates; the 0 / 10 / 25 / 50 % points of 10 log10 ZH: c1_rain_rhi 51.4 / 52.1 / 52.2 / 52.4, c2_rsg 16.6 / 16.7 / 17.0 /
17.9, c3_melt_ice 24 / 52.6 / 54.4 / 55.5, d3_rsg 16.6 / 16.7 / 17.3 / 18.3 dBZ): it censors a tenth to a quarter of the gates."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_gpu_ensemble import FIELDS, GEOM, case, load, operator

pytestmark = pytest.mark.gpu

N_GATES = 70
SETS = {'c1_rain_rhi': 52.15, 'c2_rsg': 16.9, 'c3_melt_ice': 53.5, 'd3_rsg': 17.0}     # case -> sensitivity, dBZ at every range
RAIN = {'c2_rsg': np.float32(0.01), 'd3_rsg': np.float32(0.01)}                        # case -> what QR_v is scaled by
SUBBEAMS = {1: (1, 1), 3: (3, 1), 9: (3, 3)}
EVERY = ('ZH', 'ZV', 'ZDR', 'KDP', 'RHOHV', 'DELTA_HV', 'ATT_H', 'ATT_V')
SERIES = [0.0, 600.0, 1500.0]


def SP():
    from cosmo_pol_amd import species
    return species


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != 'f':
        assert np.array_equal(got, want), what
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, int((np.isnan(got) != nan).sum()))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    a, b = np.ascontiguousarray(got).view(u)[~nan], np.ascontiguousarray(want).view(u)[~nan]
    assert np.array_equal(a, b), (what, int((a != b).sum()), a.size)


def setup(name, n_sub, attenuation):
    """(config overrides, luts, cubes, three azimuths, elevations) of `name` cut to 70 gates, with the sub-beams, the attenuation
    switch and the constant sensitivity of the case."""
    conf, luts, cubes, az, el = case(name)
    conf = copy.deepcopy(conf)
    conf['radar']['range'] = N_GATES * conf['radar']['radial_resolution']
    conf['radar']['sensitivity'] = float(SETS[name])
    nh, nv = SUBBEAMS[n_sub]
    conf.setdefault('integration', {}).update({'nh_GH': nh, 'nv_GH': nv, 'weight_threshold': 1.})
    conf.setdefault('microphysics', {})['with_attenuation'] = int(attenuation)
    if name in RAIN:
        cubes = [dict(c, data=dict(c['data'], QR_v=(c['data']['QR_v'] * RAIN[name]).astype(np.float32))) for c in cubes]
    return conf, luts, cubes, az[0] + np.array([0.0, 0.5, 1.0]), np.full(3, el[0])


def arrays(res):
    return {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}


def check_case(make_op, plain, with_species, n_sub, rain_alone, attenuation, min_species, what):
    """make_op() -> a loaded operator; plain(op) / with_species(op, spec) -> the results of the two calls."""
    sp = SP()
    spec = sp.Species(fields=EVERY, dominant=True, raw=True)
    # the plain call of an operator that was never asked for species, and its launch forms
    op = make_op()
    ref = arrays(plain(op))
    forms_ref = op._ctx.launch_forms()
    op.close()
    # the same sweep in a debug context: the per-species rows
    op = make_op()
    op._ctx.enable_debug()
    plain(op)
    hl = list(op._staged_hydro)
    rows = op._ctx.debug_read('sz_integ', (3, N_GATES, len(hl), 12), np.float32)
    op.close()
    # the species call, and the plain call behind it
    op = make_op()
    res = with_species(op, spec)
    forms = op._ctx.launch_forms()
    behind = arrays(plain(op))
    forms_behind = op._ctx.launch_forms()
    consts = sp.constants_of(float(op.constants.WAVELENGTH), float(op.config['radar']['K_squared']))
    op.close()
    got = res['species']
    assert res['n_sub'] == n_sub and res['ZH'].shape == (3, N_GATES)
    assert got['names'] == tuple(hl) and got['sz'].shape == (3, N_GATES, len(hl), 12)
    # (a)
    keys = [k for k in FIELDS + GEOM if k in ref]
    assert set(k for k in FIELDS if k in ref) >= {'ZH', 'ZV', 'ZDR', 'KDP', 'PHIDP', 'mask'}
    for k in keys:
        same_bits(np.array(res[k]), ref[k], (what, 'species call', k))
        same_bits(behind[k], ref[k], (what, 'plain call behind it', k))
    # (b)
    same_bits(got['sz'], rows, (what, 'sz'))
    # (c)
    want = sp.fields_of(got['sz'], np.array(res['ZH']), *consts)
    for k in EVERY + ('dominant', 'present', 'share'):
        same_bits(got[k], want[k], (what, k))
    # (d)
    if rain_alone and not attenuation:
        for k in EVERY:
            same_bits(got[k][0], ref[k], (what, 'rain alone', k))
    # (e)
    assert forms['gate1'] == 0 and forms['gate1_ray'] == 0 and forms['graph_replayed'] == 0, forms
    assert forms['n_sub'] == n_sub and forms['subbeam_sum'] == int(n_sub >= 4), forms
    assert forms_behind == forms_ref, (forms_behind, forms_ref)
    if n_sub == 1 and forms_ref['gate1']:
        assert forms != forms_ref           # (the fast path would have taken the plain sweep)
    # not vacuous
    n_finite = int(np.isfinite(got['ZH']).sum())
    assert n_finite >= min_species, (what, n_finite)
    censored = np.isnan(res['ZH']) & np.isfinite(got['ATT_H']).any(axis=0)
    assert censored.sum() >= 1 and (got['present'][censored] == 0).all() and (got['dominant'][censored] == 255).all(), what
    assert np.isfinite(res['ZH']).sum() >= 3 * N_GATES // 2, what
    if not rain_alone:
        assert len(set(got['dominant'].ravel()) - {255}) >= 2, (what, set(got['dominant'].ravel()))
    return got


@pytest.mark.parametrize('attenuation', [1, 0])
@pytest.mark.parametrize('n_sub', [1, 3, 9])
@pytest.mark.parametrize('name', ['c1_rain_rhi', 'c2_rsg', 'c3_melt_ice'])
def test_species_sweep(name, n_sub, attenuation):
    conf, luts, cubes, az, el = setup(name, n_sub, attenuation)

    def make_op():
        op = operator(conf, luts)
        load(op, cubes[0])
        return op
    got = check_case(make_op, lambda op: op.simulate_rays(az, el), lambda op, spec: op.simulate_rays_species(az, el, spec),
                     n_sub, name == 'c1_rain_rhi', attenuation, 100, (name, n_sub, attenuation))
    if name == 'c1_rain_rhi':
        assert np.isnan(got['ZH'][1:]).all() and set(got['present'].ravel()) <= {0, 1}
    if name == 'c3_melt_ice':
        assert len(got['names']) == 6 and (got['present'] >> 3).any()         # (a melting species contributes)


def test_species_sweep_doppler_scheme_3():
    conf, luts, cubes, az, el = setup('d3_rsg', 1, 1)
    assert conf['doppler']['scheme'] == 3

    def make_op():
        op = operator(conf, luts)
        load(op, cubes[0])
        return op
    check_case(make_op, lambda op: op.simulate_rays(az, el), lambda op, spec: op.simulate_rays_species(az, el, spec),
               1, False, 1, 100, 'd3_rsg')


def test_species_time_blended():
    conf, luts, cubes, az, el = setup('c2_rsg', 1, 1)
    times = np.array([0.0, 200.0, 900.0])                   # a state itself; between the first two; between the last two

    def make_op():
        op = operator(conf, luts)
        op.load_model_series([c['data'] for c in cubes], SERIES, cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
        return op
    check_case(make_op, lambda op: op.simulate_rays_at(az, el, times), lambda op, spec: op.simulate_rays_at_species(az, el, times, spec),
               1, False, 1, 100, 'timed')


def test_only_what_is_asked_for_and_scans():
    conf, luts, cubes, az, el = setup('c2_rsg', 1, 1)
    sp = SP()
    op = operator(conf, luts)
    load(op, cubes[0])
    full = op.simulate_rays_species(az, el, sp.Species(fields=EVERY, dominant=True, raw=True))
    part = op.simulate_rays_species(az, el, sp.Species(fields=('KDP',), dominant=False), keep_gates=False)
    assert sorted(part['species']) == ['KDP', 'names'] and 'ZH' not in part
    same_bits(part['species']['KDP'], full['species']['KDP'], 'KDP alone')
    dom = op.simulate_rays_species(az, el, sp.Species(fields=(), dominant=True))
    assert sorted(dom['species']) == ['dominant', 'names', 'present', 'share']
    for k in ('dominant', 'present', 'share'):
        same_bits(dom['species'][k], full['species'][k], k)
    scans = op.get_PPI_species([float(el[0])], sp.Species(), azimuths=az)
    assert len(scans) == 1
    for k in ('ZH', 'ZDR', 'KDP', 'dominant', 'present', 'share'):
        same_bits(np.array(scans[0]['species'][k]), full['species'][k], ('PPI', k))
    rhi = op.get_RHI_species([float(az[0])], sp.Species(fields=('ZH',)), elevations=el[:1])
    same_bits(np.array(rhi[0]['species']['ZH'])[:, 0], full['species']['ZH'][:, 0], 'RHI')
    op.close()


def test_refusals_leave_the_context_usable():
    from cosmo_pol_amd import _native as N
    conf, luts, cubes, az, el = setup('c2_rsg', 1, 1)
    sp = SP()
    spec = sp.Species()
    op = operator(conf, luts)
    op.load_model_series([c['data'] for c in cubes], SERIES, cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    ref = arrays(op.simulate_rays(az, el))

    def usable():
        again = arrays(op.simulate_rays(az, el))
        for k in ('ZH', 'ZDR', 'KDP', 'PHIDP'):
            same_bits(again[k], ref[k], k)

    class Tampered(sp.Contributions):
        """The product object with what its own checks would refuse let through to the library."""
        refuses = {}
        wrong_hydro = no_arrays = second = False

        def attach(self, native, az, n_gates, n_members, *rest):
            structs, keep = sp.Contributions.attach(self, native, az, n_gates, None, *rest)
            if self.wrong_hydro:
                self.sp.n_hydro += 1
            if self.second:
                so = native.Superob()
                so.ray_window = so.gate_window = 1
                so.min_valid_fraction = 1.0
                self.so_out = np.zeros((3, N_GATES), dtype=np.float32)
                so.ZH = self.so_out.ctypes.data
                structs['superob'] = so
            return structs, keep

        def arrays(self):
            return [] if self.no_arrays else sp.Contributions.arrays(self)

    def tampered(**kw):
        p = Tampered(spec, op._staged_hydro)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    # the Python exceptions
    with pytest.raises(ValueError, match='no ensemble call'):
        op._ensemble_rays(az, el, [0, 1], None, True, 0, 'shared', False, product=sp.Contributions(spec, op._staged_hydro))
    with pytest.raises(NotImplementedError, match='process group'):
        sp.Contributions(spec, op._staged_hydro, distributed=True)
    with pytest.raises(ValueError, match='a cosmo_pol_amd.species.Species'):
        op.simulate_rays_species(az, el, ('ZH',))
    usable()
    # the library's: CPOL_ERR_ARG each, nothing queued
    with pytest.raises(ValueError, match='not by the ensemble form'):
        op._ensemble_rays(az, el, [0, 1], None, True, 0, 'shared', False, product=tampered())
    usable()
    with pytest.raises(ValueError, match='n_hydro must equal the staged hydrometeor slots'):
        op._simulate_rays(az, el, product=tampered(wrong_hydro=True))
    usable()
    with pytest.raises(ValueError, match='every output pointer is NULL'):
        op._simulate_rays(az, el, product=tampered(no_arrays=True))
    usable()
    with pytest.raises(ValueError, match='cpol_species: not together with another product in one call'):
        op._simulate_rays(az, el, product=tampered(second=True))
    usable()
    o = N.Outputs()
    s = N.Context.species_struct(3)
    o.species = C.pointer(s)
    with pytest.raises(ValueError, match=r'cpol_run_columns: hydrometeor contributions \(outputs->species\)'):
        op._ctx.run_columns(N.SweepParams(), N.Columns(), o)
    usable()
    # ... and a species call still runs
    res = op.simulate_rays_species(az, el, spec)
    same_bits(np.array(res['ZH']), ref['ZH'], 'ZH after the refusals')
    assert np.isfinite(res['species']['ZH']).sum() > 100
    op.close()
