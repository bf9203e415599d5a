"""The sub-beam sums at every sub-beam count, tile shape and presence pattern (tests/_subsum.py), in every launch form.

The reference is the PLAIN form of the product itself, CPOL_SUBSUM=0: k_psd_lookup stores the 12 columns of every item and one
thread of k_final walks the sub-beams in order.  The fixture `expected` pins that walk to the definition first --
accumulate(item_res, presence, weights) == sz_integ, bit for bit, on every case -- so sz_integ of the plain form is the
definition applied to the device's own terms, and every other form must give those bits: sz_integ, every output field, the mask.
The plain form itself meets the oracle at the suite's tolerances on sampled rays (test_reference_meets_the_oracle); bit
equality is what sees a form that adds two sub-beams in the wrong order, the oracle comparison what sees a wrong term.

Tried against scratch builds with one edit each (none touches the chain form's turn counter):
  * `sub_w[lane]` for `sub_w[s_lo + lane]` in subbeam_sum_body: the six one-wavefront forms fail, first at 65 sub-beams (every count
    up to 64 passes), and so does the Doppler test at 65; the team and chain forms (their own copy of the line) pass;
  * the barrier team form adding a round's sub-beams from the highest bit down: team2 ... team7 fail at the first case of 4
    sub-beams, in the last bit of a tenth of the entries -- while the same build meets the oracle at 1e-5 on all 18 rays: why the
    reference has to be bitwise;
  * k_final's RVEL remainder loop starting at s_done + 1: every form still equals the plain form (they share k_final) and
    test_reference_meets_the_oracle fails on RVEL at 4 sub-beams (4 % 7 != 0), the Doppler test likewise."""
import numpy as np
import pytest

import _cases
import _subsum as S
from cosmo_pol_oracle import beam, scatter
from cosmo_pol_oracle import config as ocfg

pytestmark = pytest.mark.gpu

RTOL = 1e-5
FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL']
KNOBS = ('CPOL_SUBSUM', 'CPOL_SUBSUM_COOP', 'CPOL_SUBSUM_SMALL', 'CPOL_SUBSUM_COOP_ROUNDS', 'CPOL_SUBSUM_FORM', 'CPOL_SUBSUM_TEAM',
         'CPOL_SUBSUM_CHAIN', 'CPOL_FUSE_CLASSIFY', 'CPOL_LOOKUP_LIST', 'CPOL_GATE1', 'CPOL_RARE_DIRECT', 'CPOL_PSD_RARE', 'CPOL_USE_GRAPH')
FORMS = ['default', 'gather1', 'gather', 'lds', 'scalar', 'tail', 'rounds0'] + ['team%d' % w for w in range(2, 8)] + \
        ['chain%d' % w for w in range(2, 9)]
COOP_ROUNDS = 6                                  # the default of CPOL_SUBSUM_COOP_ROUNDS: blocks through LDS before the gather tail


def form_env(form):
    """The environment of a launch form, as tests/test_gpu_fullsize.py::test_c4_sector_with_49_subbeams_vs_oracle sets it (every knob
    is read when the context is created).  'gather': the small-launch experiment (three wavefronts per (tile, species));
    'gather1': one wavefront, the per-lane gather; 'lds' / 'scalar': up to six table blocks per sub-beam through LDS / the scalar
    cache, the rest by the gather tail; 'tail' / 'rounds0': one / no block that way; 'team<W>': W wavefronts, a barrier per round;
    'chain<W>': W wavefronts, the float32 sums handed on in LDS behind a turn counter; 'default': what the host picks."""
    if form == 'default':
        return {}
    if form == 'plain':
        return {'CPOL_SUBSUM': '0'}
    team = form[4:] if form.startswith('team') else form[5:] if form.startswith('chain') else '0'
    return {'CPOL_SUBSUM_COOP': '0' if form.startswith('gather') else '1',
            'CPOL_SUBSUM_SMALL': '0' if form == 'gather1' else '1',
            'CPOL_SUBSUM_COOP_ROUNDS': '1' if form == 'tail' else '0' if form == 'rounds0' else str(COOP_ROUNDS),
            'CPOL_SUBSUM_FORM': 'scalar' if form == 'scalar' else 'lds',
            'CPOL_SUBSUM_TEAM': team,
            'CPOL_SUBSUM_CHAIN': '1' if form.startswith('chain') else '0'}


def _config(melt=True, doppler=1):
    over = _cases.gen_golden.radial_case_inputs('c4_7x7')[0]
    over = {k: dict(v) for k, v in over.items()}
    over['microphysics'].update(with_melting=int(melt), with_ice_crystals=int(melt))
    over['doppler']['scheme'] = doppler
    conf = ocfg.make_config(over)
    hl = ocfg.hydrometeor_list(conf)
    assert tuple(hl) == (S.SPECIES if melt else S.SPECIES_DRY)
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in hl}
    return over, conf, luts


def _operator(form, over, luts):
    from cosmo_pol_amd import RadarOperator
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in form_env(form).items():
            mp.setenv(k, v)
        op = RadarOperator(config=over, luts=luts, output_variables='only_radar')
    op._ctx.enable_debug(True)                   # (keeps sz_integ readable; the sums' launch forms do not depend on it)
    return op


def _run(op, case):
    cols = S.make_columns(case)
    res = op.simulate_columns(dict(cols))
    assert res['n_sub'] == case.n_sub and res['ZH'].shape == (case.n_rays, case.n_gates)
    out = {k: res[k] for k in FIELDS + ['mask']}
    out['sz_integ'] = op._ctx.debug_read('sz_integ', (case.n_rays, case.n_gates, len(case.species), 12), np.float32)
    out['forms'] = op._ctx.launch_forms()
    return out


def _same(a, b):
    """Equal bits where neither is NaN, NaN at the same places."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(u), b[~nb].view(u))


def _where(a, b):
    d = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    w = np.argwhere(d)
    return '%d of %d differ, first at %s: %r against %r' % (len(w), a.size, w[0].tolist(), a[tuple(w[0])], b[tuple(w[0])])


def _assert_equal_bits(got, ref, tag):
    for k in ['sz_integ'] + FIELDS + ['mask']:
        assert _same(got[k], ref[k]), '%s: %s: %s' % (tag, k, _where(got[k], ref[k]))


def _pin_plain_walk(op, case, out):
    """accumulate(item_res, presence, weights) == sz_integ bit for bit, presence == the device's keys; -> the number of distinct
    (key, panel) blocks per (species on a 1-D table, tile, sub-beam with work), and the items outside the tables."""
    cols = S.make_columns(case)
    pres = S.presence(case, cols)
    nh, nr, ns, ng = len(case.species), case.n_rays, case.n_sub, case.n_gates
    res = op._ctx.debug_read('item_res', (nh, nr, ns, ng, 12), np.float64)
    key = op._ctx.debug_read('item_key', (nh, nr, ns, ng), np.int32)
    rec = op._ctx.debug_read('item_rec', (nh, nr, ns, ng, 2), np.float64)
    present = np.stack([pres[h] for h in case.species])                      # [nh, nr, ns, ng]
    assert np.array_equal(key >= 0, present), '%s: the device holds other items than the columns say' % case.name
    terms = np.where(present[..., None], res, 0.0).transpose(2, 1, 3, 0, 4)    # [ns, nr, ng, nh, 12]
    w = cols['quad_weights']
    w = w.transpose(1, 0, 2) if np.ndim(w) == 3 else w
    want = S.accumulate(terms, present.transpose(2, 1, 3, 0), w)
    assert _same(out['sz_integ'], want), '%s: the plain walk of k_final against the definition: %s' % (
        case.name, _where(out['sz_integ'], want))
    cnt = op._ctx.counters()
    assert cnt.n_valid_items == int(present.sum()) and cnt.n_subbeam_gates == nr * ns * ng
    # distinct blocks per tile and sub-beam, species on 1-D tables (the melting species walk 2-D tables in k_psd_lookup)
    tile, _ = case.tile_index()
    blocks = []
    for j, h in enumerate(case.species):
        if h in ('mS', 'mG'):
            continue
        on = present[j] & (rec[j, ..., 0] >= 0)
        ident = np.where(on, key[j].astype(np.int64) * 65536 + np.floor(np.where(on, rec[j, ..., 0], 0.0)).astype(np.int64), -1)
        for t in np.unique(tile):
            ids = np.sort(ident.transpose(1, 0, 2)[:, tile == t], axis=1)   # [ns, lanes]
            n = (ids[:, 0] >= 0).astype(int) + ((ids[:, 1:] != ids[:, :-1]) & (ids[:, 1:] >= 0)).sum(axis=1)
            blocks.append(n[n > 0])
    return np.concatenate(blocks) if blocks else np.zeros(0, int), int(cnt.n_valid_items - cnt.n_table_items), int(cnt.n_valid_items)


@pytest.fixture(scope='module')
def setup():
    return _config()


@pytest.fixture(scope='module')
def expected(setup):
    """{case name: outputs of the plain form}, each pinned to the definition; with the coverage that needs the device's keys."""
    over, conf, luts = setup
    op = _operator('plain', over, luts)
    ref, blocks, n_off, n_valid = {}, [], 0, 0
    for case in S.CASES:
        out = _run(op, case)
        assert out['forms']['subbeam_sum'] == 0 and out['forms']['final_inplace'] == 0, (case.name, out['forms'])
        b, off, valid = _pin_plain_walk(op, case, out)
        blocks.append(b)
        n_off += off
        n_valid += valid
        ref[case.name] = out
    op.close()
    blocks = np.concatenate(blocks)
    print('plain form: %d cases, %d items (%d outside the tables); distinct blocks per (species, tile, sub-beam): 1 x %d, > %d x %d, most %d'
          % (len(ref), n_valid, n_off, (blocks == 1).sum(), COOP_ROUNDS, (blocks > COOP_ROUNDS).sum(), blocks.max()))
    assert (blocks > COOP_ROUNDS).any(), 'no tile and sub-beam with more blocks than the cooperative rounds: the gather tail never runs'
    assert (blocks == 1).any()
    assert n_off > 0, 'no item outside the integral tables'
    assert n_valid - n_off > 10 * n_off, 'most items must sit on the tables'
    n_finite = sum(int(np.isfinite(o['sz_integ']).sum()) for o in ref.values())
    assert n_finite > 100000, n_finite
    return ref


@pytest.mark.parametrize('form', FORMS)
def test_form_gives_the_reference_bits(setup, expected, form):
    over, conf, luts = setup
    op = _operator(form, over, luts)
    seen = {}
    try:
        for case in S.CASES:
            got = _run(op, case)
            f = got['forms']
            seen[(f['subbeam_sum'], f['final_inplace'])] = seen.get((f['subbeam_sum'], f['final_inplace']), 0) + 1
            if case.n_sub >= 4:
                assert f['subbeam_sum'] == 1 and f['final_inplace'] == 0, (form, case.name, f)
            else:
                # (2 and 3 sub-beams with melting species: neither a sum kernel nor the in-place evaluation -- k_psd_lookup runs for
                # the melting species anyway and keeps storing the columns; rain, snow and graupel alone:
                # test_two_and_three_subbeams_in_place)
                assert f['subbeam_sum'] == 0, (form, case.name, f)
            _assert_equal_bits(got, expected[case.name], '%s %s' % (form, case.name))
    finally:
        op.close()
    print('%s: %s -> (subbeam_sum, final_inplace): cases %s' % (form, form_env(form), seen))


def test_two_and_three_subbeams_in_place():
    """Rain, snow and graupel alone: k_final evaluates the table items of 2 and 3 sub-beams in place (final_inplace; with
    melting species or, under Doppler, ice crystals the launch sequence keeps k_psd_lookup and its stored columns): against the
    plain form, which is pinned to the definition here as well."""
    over, conf, luts = _config(melt=False)
    plain, inplace = _operator('plain', over, luts), _operator('default', over, luts)
    try:
        for case in S.DRY_CASES:
            ref = _run(plain, case)
            assert ref['forms']['final_inplace'] == 0 and ref['forms']['subbeam_sum'] == 0
            _pin_plain_walk(plain, case, ref)
            got = _run(inplace, case)
            assert got['forms']['final_inplace'] == 1 and got['forms']['subbeam_sum'] == 0, (case.name, got['forms'])
            _assert_equal_bits(got, ref, 'in place ' + case.name)
            assert np.isfinite(ref['sz_integ']).sum() > 100
    finally:
        plain.close()
        inplace.close()


def _pick(prefix, wgate=False):
    names = [c.name for c in S.CASES if c.name.startswith(prefix + '_p') and c.wgate == wgate]
    assert len(names) == 1, (prefix, names)
    return S.BY_NAME[names[0]]


def _against_oracle(out, case, ray, conf, ol, tag):
    from test_gpu_seam import _tol
    o = scatter.radar_observables(S.oracle_subbeams(case, S.make_columns(case), ray), ol, conf, return_sz=True)
    _cases.assert_close_nan(out['sz_integ'][ray], o.sz_integ, rtol=RTOL, name=tag + 'sz_integ')
    sz = np.nan_to_num(o.sz_total.astype(np.float64))
    for k in FIELDS:
        atol = 2e-4 if k == 'RVEL' else _tol(tag, k, sz, conf)
        _cases.assert_close_nan(out[k][ray], o.values[k], rtol=RTOL, atol=atol, name=tag + k)
    assert np.array_equal(out['mask'][ray], o.mask), tag
    return int(np.isfinite(o.sz_integ).sum()), int(np.isfinite(o.values['RVEL']).sum())


def test_reference_meets_the_oracle(setup, expected):
    over, conf, luts = setup
    ol = {h: _cases.as_oracle_lut(l) for h, l in luts.items()}
    n_sz = n_rvel = 0
    for case in (_pick('s4_r17_g5'), _pick('s9_r17_g5'), _pick('s65_r17_g5'), _pick('s130_r3_g31'), _pick('s49_r33_g6'),
                 _pick('s65_r17_g5', wgate=True)):
        for ray in (0, case.n_rays // 2, case.n_rays - 1):
            a, b = _against_oracle(expected[case.name], case, ray, conf, ol, '%s ray %d: ' % (case.name, ray))
            n_sz += a
            n_rvel += b
    # one ray each at further counts: with those above, every remainder of k_final's groups of 7 sub-beams (RVEL terms, mask codes),
    # which all forms share -- the bitwise comparison cannot see them
    more = [_pick('s%d_r17_g5' % n) for n in (5, 6, 7, 8, 17)]
    assert set(c.n_sub % 7 for c in more) | {4 % 7, 9 % 7, 49 % 7} == set(range(7))
    for case in more:
        _against_oracle(expected[case.name], case, 11, conf, ol, '%s ray 11: ' % case.name)
    assert n_sz > 2000 and n_rvel > 100, (n_sz, n_rvel)


def test_doppler_sums_written_by_the_sum_kernels():
    """Doppler scheme 2 with 1-moment ice: the table of the ice crystals carries the Doppler sums, and the sum kernels write them
    (want_vn) for k_final's RVEL."""
    over, conf, luts = _config(doppler=2)
    ol = {h: _cases.as_oracle_lut(l) for h, l in luts.items()}
    plain = _operator('plain', over, luts)
    ref = {}
    try:
        for case in S.DOPPLER_CASES:
            ref[case.name] = _run(plain, case)
            _pin_plain_walk(plain, case, ref[case.name])
            assert np.isfinite(ref[case.name]['RVEL']).sum() > case.n_rays * case.n_gates // 2
            ray = case.n_rays // 2
            _against_oracle(ref[case.name], case, ray, conf, ol, 'Doppler scheme 2 %s ray %d: ' % (case.name, ray))
    finally:
        plain.close()
    assert any(S.presence(c, S.make_columns(c))['I'].any() for c in S.DOPPLER_CASES)
    for form in ('gather1', 'lds', 'team4', 'chain4'):
        op = _operator(form, over, luts)
        try:
            for case in S.DOPPLER_CASES:
                got = _run(op, case)
                assert got['forms']['subbeam_sum'] == 1, (form, case.name, got['forms'])
                _assert_equal_bits(got, ref[case.name], 'Doppler scheme 2 %s %s' % (form, case.name))
        finally:
            op.close()


def test_81_subbeams_through_the_configuration():
    """nh_GH = nv_GH = 9 is an ordinary configuration: 81 sub-beams, the second chunk of validity bits, through simulate_rays."""
    from cosmo_pol_amd import RadarOperator
    from test_gpu_parity import _pol_tolerances
    over, az0, el0, cube, two = _cases.gen_golden.radial_case_inputs('c4_7x7')
    over = {k: dict(v) for k, v in over.items()}
    over['integration'].update(nh_GH=9, nv_GH=9, weight_threshold=1.)
    over['radar'].update(range=12000, radial_resolution=600)
    conf = ocfg.make_config(over)
    hl = ocfg.hydrometeor_list(conf)
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in hl}
    ocube = beam.ModelCube({n: cube['data'][n].copy() for n in _cases.ORDER}, cube['zlevels'], cube['proj_info'],
                           cube['resolution'], _cases.ORDER)
    ol = {h: _cases.as_oracle_lut(l) for h, l in luts.items()}
    az = az0 + 1.5 * np.arange(17)
    el = np.full(17, el0)
    out = {}
    for form in ('default', 'plain'):
        with pytest.MonkeyPatch.context() as mp:
            for k in KNOBS:
                mp.delenv(k, raising=False)
            for k, v in form_env(form).items():
                mp.setenv(k, v)
            op = RadarOperator(config=over, luts=luts, output_variables='only_radar')
        op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
        out[form] = op.simulate_rays(az, el, apply_sensitivity=False)
        forms = op._ctx.launch_forms()
        assert out[form]['n_sub'] == 81 and forms['n_sub'] == 81
        assert forms['subbeam_sum'] == (1 if form == 'default' else 0), forms
        op.close()
    res = out['default']
    assert res['ZH'].shape == (17, 20)
    for k in FIELDS + ['mask']:
        assert _same(res[k], out['plain'][k]), '%s: %s' % (k, _where(res[k], out['plain'][k]))
    n_valid = 0
    for r in (3, 16):
        subs = beam.interpolate_radial(ocube, conf, float(az[r]), float(el[r]))
        assert len(subs) == 81
        o = scatter.radar_observables(subs, ol, conf, return_sz=True)
        szt = np.nan_to_num(o.sz_total.astype(np.float64))
        assert np.array_equal(res['mask'][r], o.mask)
        for k in FIELDS:
            atol = 2e-4 if k == 'RVEL' else _pol_tolerances(k, o, szt, conf)
            _cases.assert_close_nan(res[k][r], o.values[k], rtol=1e-5, atol=atol, name='%s ray %d' % (k, r))
        n_valid += int(np.isfinite(o.values['ZH']).sum())
    assert n_valid > 20, n_valid
