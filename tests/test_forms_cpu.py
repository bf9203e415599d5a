"""The launch rules of a sweep (cosmo_pol_amd/csrc/cpol_forms.h: choose_forms, knobs_from_env) on the host, through
tests/c_host/forms_check.cpp.  No expected value here comes from choose_forms itself:

1. Recorded forms.  launch_forms() dictionaries recorded on an MI355X by earlier commits (profiles/r6_bench_line.json,
   profiles/timed_profile.json, profiles/superob_profile.json) and the expectations the GPU tests assert (FORMS of
   tests/test_gpu_scans.py, read from its source; test_gpu_timed.py::test_launch_forms, test_gpu_gate_tiles.py, test_gpu_levels.py,
   test_gpu_seam.py, test_gpu_edges.py, test_gpu_subsum.py, copied below with their origin).  Each call is described from the profile's own
   record or the test's setup -- shape, species, lanes, entry point, environment -- and the entries that record names must come out.
   `graph_replayed` is decided after the launch and is not compared.

2. Implications over an enumerated input space (forms_check implications: n_sub 1 / 3 / 4, n_rays 1 / 15 / 16 / 300 / 70000, n_gates
   1 / 64 / 65, every entry point, debug reads, Doppler 0-3, melting, lanes 0 / 2, all 1-D tables / one 2-D table / one slot without a
   table, every knob at every documented value one at a time, and the remaining inputs one at a time).  Each was read off run_sequence
   as it stood before the rules moved (cosmo_pol_hip.hip at commit 89669c7, line numbers of that file):
     gate1 => n_sub == 1, final_inplace, rare_direct                          2447-2450 (n_sub == 1; final_inplace set), 2492-2493
     gate1_ray => gate1, no melting, not Doppler 2, n_rays <= 65535           2463
     gate1_ray => by_species (the rule once written twice)                    2471-2472 against 2968-2971; k_gate1_ray launched at 2971
     by_species => gate1, not fused_gate1; fused_gate1 => gate1               2946 (the branch), 2969-2970, 2508
     fused => rare_direct, not gate1, not columns / export / members          2503
     subsum => n_sub >= 4; final_inplace without gate1 => n_sub < 4           2430, 2435
     never subsum and final_inplace (gate1 needs n_sub == 1, so not then either)   2430, 2435, 2447-2450
     rare_direct => every slot has a table                                    2492-2493
     Doppler 3 => none of gate1, subsum, fused (nor k_rvel_terms)             2422, 2447, 2503 (2357, 3407 with 3331)
     poly_single => no k_trajectory preparation (n_sub < 4), not columns, ground 4/3 geometry, no site table, a version tag   2190, 2200-2201
       (the rule says "not ray_prep", which is n_sub < 4, not n_sub == 1: with 2 or 3 sub-beams the central one takes the polynomials)
     stencil => no graph, nz < 32768, one sub-beam, the plain k_interp_sweep launch   2714, 2721-2722
     graphable => CPOL_USE_GRAPH, none of columns / export / members / Doppler 3      3433-3434
     present => gate1_ray, not columns / members                              2662
     the rest (psd_rare_one, rare_fork, use_tile_list) => rare_direct, not gate1      3165, 3101-3105, 2905

3. Knob parsing: knobs_from_env() in a child process per environment: the clamps, the two string matches, and the defaults, which are
   the initialisers cpol_ctx had (copied below from that struct)."""
import ast
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB_ENV = ('CPOL_USE_GRAPH', 'CPOL_SUBSUM_COOP', 'CPOL_LOOKUP_LIST', 'CPOL_LOOKUP_SPLIT', 'CPOL_GATE1_SPECIES', 'CPOL_GATE1_RAY',
            'CPOL_FUSE_GATE1', 'CPOL_FUSE_CLASSIFY', 'CPOL_RARE_OVERLAP', 'CPOL_RARE_DIRECT', 'CPOL_GATE1', 'CPOL_SUBSUM', 'CPOL_SUBSUM_FORM',
            'CPOL_SUBSUM_CHAIN', 'CPOL_SUBSUM_TEAM', 'CPOL_SUBSUM_SMALL', 'CPOL_TABLE_UPLOAD', 'CPOL_GEO_POLY_CENTRAL', 'CPOL_GEO_POLY',
            'CPOL_PSD_RARE', 'CPOL_SUBSUM_COOP_ROUNDS')
PROCESS_ENV = ('CPOL_GATE1_PRESENT', 'CPOL_EXP_SKIP', 'CPOL_LOOKUP_TILE', 'CPOL_LOOKUP_FILL', 'CPOL_ICE_FORCE_SUM', 'CPOL_PSD_ONLY',
               'CPOL_PSD_GRID', 'CPOL_PSD_GRID_GENERIC', 'CPOL_PSD_SIBLINGS', 'CPOL_PSD_LDS_PAD', 'CPOL_FINAL_512')
# the initialisers of cpol_ctx's knob fields before they became struct Knobs, and of the `static const` reads of run_sequence
DEFAULTS = {'use_graph': 0, 'subsum_coop_rounds': 6, 'rare_overlap': 0, 'rare_direct': 1, 'lookup_list': 1, 'lookup_split': 0, 'gate1_ray': -1,
            'gate1_species': 1, 'fuse_gate1': 0, 'fuse_classify': 1, 'gate1': 1, 'subsum': 1, 'subsum_scalar': 0, 'upload_kernel': 0,
            'geo_poly_central': 1, 'geo_poly': 1, 'psd_rare': 1, 'subsum_small': 0, 'subsum_chain': 1, 'subsum_team': -1, 'subsum_coop': -1,
            'p.gate1_present': 1, 'p.exp_skip': 0, 'p.lookup_tile': 1, 'p.lookup_fill': 12, 'p.ice_force_sum': 0, 'p.psd_only': 15,
            'p.psd_grid': 1024, 'p.psd_grid_generic': 1024, 'p.psd_siblings': 0, 'p.psd_lds_pad': 0, 'p.final_512': -1}
FORM_NAMES = ('g1r', 'gate1_ray', 'gate1', 'interp_classify', 'rare_direct', 'subbeam_sum', 'final_inplace', 'poly_central', 'n_sub',
              'lanes_alive', 'scan_form')
C3 = 'R,S,G,mS,mG,I'                 # bench.py: the species of c3 / c4 (melting layer and ice crystals)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('forms') / 'forms_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'c_host', 'forms_check.cpp'), '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def _run(exe, args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in KNOB_ENV + PROCESS_ENV}
    e.update(env or {})
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _values(text):
    return {k: int(v) for k, v in (line.split('=') for line in text.split())}


def _forms(exe, env=None, **call):
    return _values(_run(exe, ['forms'] + ['%s=%s' % kv for kv in call.items()], env))


def _recorded(path, *keys):
    with open(os.path.join(ROOT, 'profiles', path)) as f:
        text = f.read()
    if path == 'r6_bench_line.json':            # ('#detail <name> {...}' sections on one line each, not one JSON document)
        m = re.search(r'"launch_forms": (\{[^}]*\})', text)
        return json.loads(m.group(1))
    d = json.loads(text)
    for k in keys:
        d = d[k]
    return d


def _scan_forms():
    """FORMS of tests/test_gpu_scans.py, from its source (importing the module would need the oracle and a GPU marker's fixtures)."""
    with open(os.path.join(ROOT, 'tests', 'test_gpu_scans.py')) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', None) == 'FORMS':
            return ast.literal_eval(node.value)
    raise AssertionError('FORMS not found in tests/test_gpu_scans.py')


def _assert_entries(got, want, tag):
    want = {k: v for k, v in want.items() if k != 'graph_replayed'}
    assert {k: got[k] for k in want} == want, (tag, got)


def test_recorded_profiles(exe):
    # bench.py's c2 headline: 360 x 500, one sub-beam, R S G, two lanes beside the root, device outputs, a version tag per elevation
    want = _recorded('r6_bench_line.json')
    assert set(want) == set(FORM_NAMES + ('graph_replayed',))
    _assert_entries(_forms(exe, lanes=want['lanes_alive'], dev=1, doppler=1), want, 'r6_bench_line')
    # tools/superob_profile.py: the same sweep with superobservations, and a members call (form B keeps every array on the device)
    for section, entry in (('sweep', 'sweep'), ('ensemble', 'members')):
        want = _recorded('superob_profile.json', section, 'launch_forms_B')
        _assert_entries(_forms(exe, lanes=want['lanes_alive'], entry=entry, dev=1, doppler=1), want, 'superob ' + section)
    # tools/timed_profile.py: time-blended sweeps of c2 (360 x 500) and of the c4 share (225 x 500, 7 x 7 sub-beams), no lanes
    for wl, species, n_h, melting in (('c2', 'R,S,G', 1, 0), ('c4', C3, 7, 1)):
        rec = _recorded('timed_profile.json', 'workloads', wl)
        got = _forms(exe, entry='timed', n_rays=rec['n_rays'], n_gates=rec['n_gates'], n_sub=rec['n_sub'], n_h=n_h, species=species,
                     with_melting=melting, doppler=1, dev=1)
        _assert_entries(got, rec['launch_forms_T'], 'timed ' + wl)


@pytest.mark.parametrize('form', ['final', 'scan_rays', 'ticket', 'general', 'general4'])
def test_scan_suite_forms(exe, form):
    """tests/test_gpu_scans.py: a columns call of 10 rays (tests/_scans.py: one per ray family), R S G without melting, Doppler
    scheme 1, under the row's environment; every gate count of its cases at which the host takes another path."""
    env, want = _scan_forms()[form]
    want = dict(want, scan_form=1)
    for n_gates in (1, 64, 65, 257, 513):
        got = _forms(exe, env, entry='columns', n_rays=10, n_gates=n_gates, n_sub=want['n_sub'], n_h=want['n_sub'], doppler=1, versioned=0)
        _assert_entries(got, want, (form, n_gates))
        assert got['interp_classify'] == 0           # (never for columns: test_gpu_seam.py)


def test_other_gpu_suites(exe):
    # test_gpu_timed.py::test_launch_forms: the radial cases c2_rsg (150 gates, one beam) and c4_7x7 (49 sub-beams) at a time between states
    got = _forms(exe, entry='timed', n_rays=2, n_gates=150, doppler=1)
    _assert_entries(got, {'n_sub': 1, 'gate1': 1, 'interp_classify': 0}, 'timed c2_rsg')
    got = _forms(exe, entry='timed', n_rays=2, n_gates=60, n_sub=49, n_h=7, species=C3, with_melting=1, doppler=1)
    _assert_entries(got, {'n_sub': 49, 'gate1': 0, 'interp_classify': 0}, 'timed c4_7x7')
    # test_gpu_gate_tiles.py: the c2 sweep and one that is no multiple of the tile, no lanes, three ways (and the ticket form)
    for shape in ((360, 500), (359, 497)):
        for env, want in (({'CPOL_GATE1_RAY': '1'}, {'gate1_ray': 1, 'gate1': 1}), ({'CPOL_GATE1_RAY': '0'}, {'gate1_ray': 0, 'gate1': 1}),
                          ({'CPOL_GATE1': '0'}, {'gate1': 0}), ({'CPOL_GATE1_RAY': '3'}, {'gate1_ray': 1, 'gate1': 1})):
            _assert_entries(_forms(exe, env, n_rays=shape[0], n_gates=shape[1], doppler=1), want, (shape, env))
    # ... tables cut to their lower panels (CPOL_ITAB_KEEP_PANELS), 23 x 131: k_gate1_ray forced by CPOL_GATE1_RAY=2
    cut = 'R~,S~,G~'
    _assert_entries(_forms(exe, {'CPOL_GATE1_RAY': '2'}, n_rays=23, n_gates=131, species=cut, doppler=1), {'gate1_ray': 1, 'gate1': 1}, 'cut / 2')
    _assert_entries(_forms(exe, {'CPOL_GATE1_RAY': '0'}, n_rays=23, n_gates=131, species=cut, doppler=1), {'gate1_ray': 0, 'gate1': 1}, 'cut / 0')
    _assert_entries(_forms(exe, {'CPOL_GATE1': '0', 'CPOL_RARE_DIRECT': '0'}, n_rays=23, n_gates=131, species=cut, doppler=1), {'gate1': 0}, 'cut / general')
    # ... and with three lanes in flight (two beside the root) against one context without lanes: the same two modes
    for lanes in (0, 2):
        _assert_entries(_forms(exe, {'CPOL_GATE1_RAY': '1'}, lanes=lanes, doppler=1, dev=1), {'gate1_ray': 1, 'gate1': 1}, lanes)
        _assert_entries(_forms(exe, {'CPOL_GATE1_RAY': '0'}, lanes=lanes, doppler=1, dev=1), {'gate1_ray': 0, 'gate1': 1}, lanes)
    # the default: k_gate1_ray with lanes, the one-lane sequence without (the headline above against the timed profile)
    assert _forms(exe, lanes=2)['gate1_ray'] == 1 and _forms(exe, lanes=0)['gate1_ray'] == 0
    # test_gpu_levels.py: a two-member ensemble of the 7 x 7 case; test_gpu_seam.py / test_gpu_levels.py: a column call never interpolates
    # and shares the other forms with the sweep of the same gates
    _assert_entries(_forms(exe, entry='members', n_rays=4, n_gates=60, n_sub=49, n_h=7, species=C3, with_melting=1), {'interp_classify': 0, 'n_sub': 49}, 'ensemble')
    shared = ('g1r', 'gate1_ray', 'gate1', 'rare_direct', 'subbeam_sum', 'final_inplace', 'n_sub')          # SHARED_FORMS of test_gpu_seam.py
    for call in (dict(n_rays=1, n_gates=150), dict(n_rays=1, n_gates=150, species=C3, with_melting=1),
                 dict(n_rays=1, n_gates=60, n_sub=49, n_h=7, species=C3, with_melting=1, doppler=1), dict(n_rays=1, n_gates=100, doppler=3),
                 dict(n_rays=1, n_gates=100, species='R,S,G,N', doppler=2)):
        sweep = _forms(exe, **call)
        for entry in ('columns', 'columns_melt') if call.get('with_melting') else ('columns',):
            cols = _forms(exe, entry=entry, versioned=0, **call)
            assert cols['interp_classify'] == 0 and {k: cols[k] for k in shared} == {k: sweep[k] for k in shared}, (call, entry, cols, sweep)
    # test_gpu_edges.py: 120 rays with device outputs under a version tag take the coordinate polynomials; CPOL_DEBUG_EXACT_SUBBEAMS does not
    assert _forms(exe, n_rays=120, n_gates=60, dev=1)['poly_central'] == 1
    assert _forms(exe, n_rays=120, n_gates=60, dev=1, exact=1)['poly_central'] == 0
    # test_gpu_subsum.py: 17 rays x 20 gates of 9 x 9 sub-beams: k_subbeam_sum by default, not with CPOL_SUBSUM=0
    assert _forms(exe, n_rays=17, n_gates=20, n_sub=81, n_h=9, species=C3, with_melting=1)['subbeam_sum'] == 1
    assert _forms(exe, {'CPOL_SUBSUM': '0'}, n_rays=17, n_gates=20, n_sub=81, n_h=9, species=C3, with_melting=1)['subbeam_sum'] == 0


def test_implications_over_the_input_space(exe):
    out = _run(exe, ['implications'])
    m = re.search(r'FORMS_IMPLICATIONS_OK (\d+)', out)
    assert m and int(m.group(1)) > 1000000, out


def test_knob_defaults_clamps_and_string_matches(exe):
    assert _values(_run(exe, ['knobs'])) == DEFAULTS
    for name, field, lo, hi in (('CPOL_GATE1_RAY', 'gate1_ray', -1, 3), ('CPOL_LOOKUP_SPLIT', 'lookup_split', 0, 16),
                                ('CPOL_LOOKUP_LIST', 'lookup_list', 0, 2), ('CPOL_SUBSUM_COOP_ROUNDS', 'subsum_coop_rounds', 0, 64),
                                ('CPOL_GATE1_SPECIES', 'gate1_species', 0, 2), ('CPOL_GEO_POLY_CENTRAL', 'geo_poly_central', 0, 2)):
        for given, want in ((lo - 5, lo), (lo, lo), (hi, hi), (hi + 5, hi), ((lo + hi) // 2, (lo + hi) // 2)):
            got = _values(_run(exe, ['knobs'], {name: str(given)}))
            assert got == dict(DEFAULTS, **{field: want}), (name, given)
    for name, field, word in (('CPOL_SUBSUM_FORM', 'subsum_scalar', 'scalar'), ('CPOL_TABLE_UPLOAD', 'upload_kernel', 'kernel')):
        assert _values(_run(exe, ['knobs'], {name: word}))[field] == 1
        for other in ('1', word.upper(), word + 's', ''):
            assert _values(_run(exe, ['knobs'], {name: other}))[field] == 0, (name, other)
    # switches are 0 / 1 whatever the number; CPOL_GATE1 and CPOL_SUBSUM_TEAM are taken as they are; CPOL_SUBSUM_COOP loses its -1
    for env, field, want in (({'CPOL_USE_GRAPH': '2'}, 'use_graph', 1), ({'CPOL_SUBSUM': '-3'}, 'subsum', 1), ({'CPOL_RARE_DIRECT': '0'}, 'rare_direct', 0),
                             ({'CPOL_GATE1': '2'}, 'gate1', 2), ({'CPOL_SUBSUM_TEAM': '8'}, 'subsum_team', 8), ({'CPOL_SUBSUM_COOP': '-1'}, 'subsum_coop', 1),
                             ({'CPOL_SUBSUM_COOP': '0'}, 'subsum_coop', 0), ({'CPOL_PSD_ONLY': '5'}, 'p.psd_only', 5), ({'CPOL_EXP_SKIP': '6'}, 'p.exp_skip', 6),
                             ({'CPOL_PSD_SIBLINGS': '1'}, 'p.psd_siblings', 1), ({'CPOL_FINAL_512': '0'}, 'p.final_512', 0),
                             ({'CPOL_LOOKUP_FILL': '24'}, 'p.lookup_fill', 24), ({'CPOL_GATE1_PRESENT': '0'}, 'p.gate1_present', 0)):
        assert _values(_run(exe, ['knobs'], env)) == dict(DEFAULTS, **{field: want}), env


# ---- the launch plan of tests/test_gpu_rvel.py, stage (E): launch_forms() names neither the k_subbeam_sum form, k_gate1_species,
# k_rvel_terms nor the width of k_final, so the GPU test asserts those runs only through their knobs.  Here the same calls -- shape,
# species, entry point, knobs -- go through choose_forms on the host: each knob set must select the form the plan names for it.
# The expectations are the enum of cpol_forms.h (SUM_GATHER 0, SUM_SMALL 1, SUM_LDS 2, SUM_SCALAR 3, SUM_TEAM 4) and the rules' own
# statements (k_rvel_terms from 4 sub-beams on; 512 threads beyond 256 gates with at most 256 rays unless CPOL_FINAL_512=0).
RVEL_SPECIES = {'rsg': 'R,S,G', 'rsgi': 'R,S,G,I', 'melt': 'R,S,G,mS,mG,I', '2mom': 'R,S,G,G,N'}
RVEL_SUM = {'default': dict(sum_form=4, sum_team=4, sum_chain=1), 'gather': dict(sum_form=0, sum_team=0), 'lds': dict(sum_form=2, sum_team=0),
            'scalar': dict(sum_form=3, sum_team=0), 'small': dict(sum_form=1, sum_team=0), 'team2': dict(sum_form=4, sum_team=2, sum_chain=1),
            'team3_barrier': dict(sum_form=4, sum_team=3, sum_chain=0), 'team8': dict(sum_form=4, sum_team=8, sum_chain=1)}
RVEL_SINGLE = {'species0': dict(by_species=0), 'species2': dict(by_species=1), 'ray0': dict(by_species=1, gate1_ray=0),
               'ray1': dict(gate1_ray=1), 'ray2': dict(gate1_ray=1), 'gate1_0': dict(by_species=0)}


def test_rvel_launch_plan_selects_the_forms_it_names(exe):
    import _rvel
    import test_gpu_rvel as T
    assert len(T.FORM_PLAN) > 50 and set(T.SUM_FORMS) == set(RVEL_SUM) - {'default'}
    seen = set()
    for name, form, knobs, want in T.FORM_PLAN:
        c = _rvel.BY_NAME[name]
        call = dict(n_rays=c.n_rays, n_gates=c.n_gates, n_sub=c.n_sub, n_h=c.n_sub, doppler=1, debug=0, ml=int(c.wgate),
                    with_melting=int(c.melt), entry='columns_melt' if c.melt else 'columns', species=RVEL_SPECIES[c.sset])
        got = _forms(exe, env={k: str(v) for k, v in knobs}, **call)
        expect = dict(want, rvel_terms=int(c.n_sub >= 4), final_512=int(c.n_gates > 256 and c.n_rays <= 256))
        if want.get('subbeam_sum'):
            expect.update(RVEL_SUM[form])
        if c.n_sub == 1 and c.sset == 'rsg':
            expect.update(RVEL_SINGLE.get(form, dict(by_species=1)))
        assert {k: got[k] for k in expect} == expect, (name, form, got)
        seen |= {(k, v) for k, v in expect.items()}
        # k_final at 256 threads, as the child of test_final_512_gives_the_same_bits runs it
        assert _forms(exe, env=dict({k: str(v) for k, v in knobs}, CPOL_FINAL_512='0'), **call)['final_512'] == 0
    for k in ('sum_form', 'sum_team'):
        assert {v for kk, v in seen if kk == k} >= {0, 2, 3, 4} if k == 'sum_team' else {v for kk, v in seen if kk == k} == {0, 1, 2, 3, 4}
    for k in ('by_species', 'gate1_ray', 'rvel_terms', 'final_512', 'sum_chain', 'final_inplace', 'gate1', 'subbeam_sum'):
        assert {v for kk, v in seen if kk == k} == {0, 1}, k
