"""k_gate1_ray's finish from the compact operand record (cosmo_pol_amd/csrc/cpol_gate_ops.h, gate_finish_single in
cpol_gate.inl): the record is filled by the host at every launch from the structs the launch passes, every vector operand
of a gate is requested in one round, and a sweep the record does not cover (`generic`) takes gate_finish as before.  None of
that may show in a single bit: the lanes path (CPOL_GATE1_RAY=1) is compared with the general sequence (CPOL_GATE1=0) on the
nine observables, RVEL and the mask through their uint32 / uint64 views, on 5 rays x 70 gates (a padding ray of the 4-ray
tile, padding gates of the 16-gate tile, two 64-gate words) of the small c2 cube and tables:
  - attenuation on and off, RVEL asked for and not, on a cube with rain, snow and graupel, one with rain alone (the wavefronts
    of the two other slots hold no item: the rain wavefront's terms alone reach the finish) and one without snow anywhere;
  - output_variables='all': model_vars is not NULL, the `generic` fall-back;
  - a Nyquist table: RVEL folded;
  - a second cube loaded into the same operator between two sweeps, and a member swap: what a fresh operator gives;
  - two operators with different table sets alive in one process, sweeping alternately.
(The operator's species list of the 1-moment scheme is always R, S, G: "rain alone" is a cube, not a one-wavefront launch.)"""
import numpy as np
import pytest

import test_gpu_gate_slots as gs

pytestmark = pytest.mark.gpu

N_RAYS, N_GATES = gs.N_RAYS, gs.N_GATES
LANES, GENERAL = gs.LANES, gs.GENERAL
CUBES = ('rsg', 'rain_alone', 'no_snow')
COMBOS = gs.COMBOS
NYQUIST = 0.6                                       # m/s: below the 0.9 to 1.9 m/s of the test cube's radial velocities, so that every gate folds


def _cubes():
    import bench
    base = bench.make_inputs('c2', True)[2]
    shape = base['data']['T'].shape
    fields = {'QR_v': gs._field(shape, 4e-4, (0.3, 0.2, 0.1)), 'QS_v': gs._field(shape, 3e-4, (-0.2, 0.1, 0.3)),
              'QG_v': gs._field(shape, 5e-4, (0.5, 0.3, 0.2))}
    zero = np.zeros(shape, dtype=np.float32)

    def cube(present):
        c = dict(base)
        c['data'] = dict(base['data'])
        for k in gs.SLOTS:
            c['data'][k] = fields[k] if k in present else zero
        return c

    return {'rsg': cube(gs.SLOTS), 'rain_alone': cube(gs.SLOTS[:1]), 'no_snow': cube((gs.SLOTS[0], gs.SLOTS[2])), 'base': base}


def _load(op, c):
    op.load_model_arrays(c['data'], c['zlevels'], c['proj_info'], c['resolution'])


def _host_sweep(op, mode):
    """a sweep with host outputs: every array of the result"""
    az, el = gs._rays()
    res = op.simulate_rays(az, el)
    forms = op._ctx.launch_forms()
    assert (forms['gate1_ray'] == 1 and forms['gate1'] == 1) if mode == 'lanes' else forms['gate1'] == 0, forms
    return {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray) and v.dtype.kind == 'f'}


def _same_arrays(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        assert np.array_equal(gs._bits(a[k]), gs._bits(b[k])), (what, k, int((gs._bits(a[k]) != gs._bits(b[k])).sum()))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    import bench
    from cosmo_pol_amd import synthetic
    luts = bench.make_inputs('c2', True)[3]
    cubes = _cubes()
    out = {}
    # ---- the cubes on ONE operator per path and attenuation setting (every load after the first replaces a cube between two
    # sweeps of the same operator); two sweeps per case on the lanes path: the stencil's full form, then recording / replay
    for att in (1, 0):
        for mode, env in (('general', GENERAL), ('lanes', LANES)):
            op = gs._operator(env, gs._conf(att), luts, cubes[CUBES[0]])
            for name in CUBES:
                if name != CUBES[0]:
                    _load(op, cubes[name])
                for rvel in (True, False):
                    out[(mode, name, att, rvel)] = [gs._sweep(op, rvel, mode)[0] for _ in range(2 if mode == 'lanes' else 1)]
            if mode == 'lanes' and att == 1:
                # a member swap on the operator that has just seen three cubes: members 0 / 1 = no_snow / rsg
                a, b = cubes['no_snow'], cubes['rsg']
                op.load_model_ensemble([a['data'], b['data']], zlevels=a['zlevels'], proj_info=a['proj_info'], resolution=a['resolution'])
                out['member0'] = gs._sweep(op, True, mode)[0]
                op.select_member(1)
                out['member1'] = gs._sweep(op, True, mode)[0]
                op.select_member(0)
                out['member0_again'] = gs._sweep(op, True, mode)[0]
            op.close()
    # ---- a fresh operator on the last cube of the walk above
    op = gs._operator(LANES, gs._conf(1), luts, cubes[CUBES[-1]])
    out['fresh'] = gs._sweep(op, True, 'lanes')[0]
    op.close()
    # ---- model_vars asked for: the generic fall-back (host outputs)
    for mode, env in (('general', GENERAL), ('lanes', LANES)):
        op = gs._operator(env, gs._conf(1), luts, cubes['rsg'], output='all')
        out[('all', mode)] = _host_sweep(op, mode)
        op.close()
    # ---- Nyquist folding
    path = tmp_path_factory.mktemp('nyquist') / 'nyquist.csv'
    path.write_text('elevation,azimuth,nyquist\n2.0,0.0,%r\n' % NYQUIST)
    conf = gs._conf(1)
    conf['radar']['nyquist_velocity'] = str(path)
    for mode, env in (('general', GENERAL), ('lanes', LANES)):
        op = gs._operator(env, conf, luts, cubes['base'])
        out[('nyquist', mode)] = gs._sweep(op, True, mode)[0]
        op.close()
    op = gs._operator(LANES, gs._conf(1), luts, cubes['base'])
    out['unfolded'] = gs._sweep(op, True, 'lanes')[0]
    op.close()
    # ---- two operators with different table sets, sweeping alternately
    luts_b = synthetic.make_all_luts(bench.hydrometeors_of('c2'), 5.6, '1mom', seed=20260302, n_e=8)
    for tag, tables in (('a', luts), ('b', luts_b)):
        op = gs._operator(GENERAL, gs._conf(1), tables, cubes['rsg'])
        out[('tables', tag, 'general')] = gs._sweep(op, True, 'general')[0]
        op.close()
    op_a = gs._operator(LANES, gs._conf(1), luts, cubes['rsg'])
    op_b = gs._operator(LANES, gs._conf(1), luts_b, cubes['rsg'])
    out[('tables', 'a', 'lanes')], out[('tables', 'b', 'lanes')] = [], []
    for _ in range(2):
        out[('tables', 'a', 'lanes')].append(gs._sweep(op_a, True, 'lanes')[0])
        out[('tables', 'b', 'lanes')].append(gs._sweep(op_b, True, 'lanes')[0])
    op_a.close()
    op_b.close()
    return out


@pytest.mark.parametrize('att,rvel', COMBOS)
@pytest.mark.parametrize('name', CUBES)
def test_record_finish_has_the_general_sequence_bits(runs, name, att, rvel):
    want = runs[('general', name, att, rvel)][0]
    for s, got in enumerate(runs[('lanes', name, att, rvel)]):
        gs._same_bits(got, want, rvel, (name, att, rvel, s))


def test_the_cases_put_values_in_front_of_the_finish(runs):
    zh = {name: np.isfinite(runs[('general', name, 1, True)][0]['ZH']) for name in CUBES}
    assert zh['rsg'].sum() > N_RAYS * N_GATES // 4 and zh['rain_alone'].sum() > N_RAYS * N_GATES // 8, {k: int(v.sum()) for k, v in zh.items()}
    rv = runs[('general', 'rsg', 1, True)][0]['RVEL']
    assert np.isfinite(rv).sum() > N_RAYS * N_GATES // 4
    # attenuation reaches the outputs through the range scans (ZDR of the attenuated reflectivities); the cubes differ
    z1, z0 = runs[('general', 'rsg', 1, True)][0]['ZDR'], runs[('general', 'rsg', 0, True)][0]['ZDR']
    assert not np.array_equal(gs._bits(z1), gs._bits(z0))
    a1 = runs[('general', 'rsg', 1, True)][0]['ZH']
    assert not np.array_equal(gs._bits(a1), gs._bits(runs[('general', 'no_snow', 1, True)][0]['ZH']))


def test_reloaded_cube_and_member_swap_equal_a_fresh_operator(runs):
    # the operator that walked rsg -> rain_alone -> no_snow against a fresh one on no_snow
    gs._same_bits(runs[('lanes', CUBES[-1], 1, True)][-1], runs['fresh'], True, 'reloaded cube')
    gs._same_bits(runs['member0'], runs['fresh'], True, 'member 0')
    gs._same_bits(runs['member1'], runs[('general', 'rsg', 1, True)][0], True, 'member 1')
    gs._same_bits(runs['member0_again'], runs['fresh'], True, 'member 0 again')


def test_model_vars_take_the_generic_finish(runs):
    a, b = runs[('all', 'lanes')], runs[('all', 'general')]
    assert 'model_vars' in a and np.isfinite(a['model_vars']).any(), sorted(a)
    _same_arrays(a, b, 'output_variables=all')


def test_nyquist_folding(runs):
    gs._same_bits(runs[('nyquist', 'lanes')], runs[('nyquist', 'general')], True, 'nyquist')
    folded, plain = runs[('nyquist', 'lanes')]['RVEL'], runs['unfolded']['RVEL']
    ok = np.isfinite(plain)
    assert np.array_equal(np.isfinite(folded), ok) and ok.sum() > N_RAYS * N_GATES // 4
    assert np.all(np.abs(folded[ok]) <= NYQUIST * (1 + 1e-12))
    assert (np.abs(plain[ok]) > NYQUIST).any() and not np.array_equal(gs._bits(folded), gs._bits(plain))


def test_two_table_sets_sweeping_alternately(runs):
    for tag in ('a', 'b'):
        for s, got in enumerate(runs[('tables', tag, 'lanes')]):
            gs._same_bits(got, runs[('tables', tag, 'general')], True, ('tables', tag, s))
    a, b = runs[('tables', 'a', 'general')]['ZH'], runs[('tables', 'b', 'general')]['ZH']
    assert not np.array_equal(gs._bits(a), gs._bits(b))
