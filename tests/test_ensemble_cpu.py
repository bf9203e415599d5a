"""Ensembles without a GPU: the C ABI of the member entry points against the header and the built library, the check that the
members of an ensemble are states of one model, and the planner that cuts a member list into chunks."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['cpol_stage_member', 'cpol_num_members', 'cpol_select_member', 'cpol_run_sweep_members']
# the library's exports on the parent commit
BEFORE = ['cpol_create', 'cpol_destroy', 'cpol_fork', 'cpol_last_error', 'cpol_set_stream', 'cpol_get_stream', 'cpol_synchronize',
          'cpol_stage_model', 'cpol_stage_hydro', 'cpol_set_num_hydro', 'cpol_stage_doppler_weights', 'cpol_stage_spectrum_tables',
          'cpol_stage_t_function', 'cpol_prepare', 'cpol_interp_points', 'cpol_ray_tables', 'cpol_run_sweep', 'cpol_interp_subbeams',
          'cpol_run_columns', 'cpol_counters', 'cpol_spaceborne_first_gate', 'cpol_host_alloc', 'cpol_host_free',
          'cpol_host_alloc_near', 'cpol_device_pci_bus_id', 'cpol_mem_info', 'cpol_enable_timing', 'cpol_debug_read',
          'cpol_debug_math', 'cpol_debug_scan', 'cpol_broaden_rows', 'cpol_stage_model_packed', 'cpol_unpack_planes']


def test_member_prototypes_match_header(tmp_path):
    """The header's prototypes are what _native.py tells ctypes: a C file that assigns every new entry point to a function
    pointer of the ctypes signature compiles without a diagnostic (-Werror); the structs they take are the sweep's, whose
    layouts tests/test_cabi_cpu.py pins."""
    import ctypes as C
    from cosmo_pol_amd import _native as N
    ctype = {C.c_void_p: 'void *', C.c_int: 'int', None: 'void'}
    # (what each void pointer of the ctypes signature is in the header)
    header_args = {
        'cpol_stage_member': 'cpol_ctx *, int, int, const float *const *',
        'cpol_num_members': 'cpol_ctx *',
        'cpol_select_member': 'cpol_ctx *, int',
        'cpol_run_sweep_members': 'cpol_ctx *, const cpol_sweep_params *, const cpol_ray_tables_t *, const int32_t *, int, cpol_outputs *',
    }
    try:
        lib = N.load_library()
    except N.NativeError:
        pytest.fail('the HIP library is not built')
    lines = ['#include "cosmo_pol_amd.h"', 'int main(void){']
    for name in NEW:
        assert name in N.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        n_args = len(header_args[name].split(','))
        assert len(fn.argtypes) == n_args, name
        for at, ha in zip(fn.argtypes, header_args[name].split(',')):
            # ints stay ints, everything else is a pointer on both sides
            assert (at is C.c_int) == (ha.strip() == 'int'), (name, at, ha)
        lines.append('{ int (*f)(%s) = %s; (void)f; }' % (header_args[name], name))
    lines.append('return 0;}')
    src = tmp_path / 'proto.c'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', '-o', str(tmp_path / 'proto.o'),
                           str(src)])
    assert N.MEMBERS_PER_CALL == 64
    text = open(os.path.join(ROOT, 'cosmo_pol_amd', 'csrc', 'cpol_members.inl')).read()
    assert re.search(r'#define CPOL_MEMBERS_PER_CALL 64\b', text)


def test_library_exports_the_member_entry_points_and_nothing_else_new():
    from cosmo_pol_amd import _native as N
    assert os.path.exists(N.LIB_PATH), 'the HIP library is not built'
    out = subprocess.check_output(['nm', '-D', '--defined-only', N.LIB_PATH]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-2] in ('T', 'W', 'B', 'D', 'V', 'R')}
    syms = {s for s in syms if not s.startswith('_') or s.startswith('_Z')}
    assert syms == set(BEFORE) | set(NEW), sorted(syms ^ (set(BEFORE) | set(NEW)))
    assert sorted(N.EXPORTS) == sorted(BEFORE + NEW)
    emap = open(os.path.join(ROOT, 'cosmo_pol_amd', 'csrc', 'exports.map')).read()
    assert 'global: cpol_*;' in emap and 'local: *;' in emap
    header = open(os.path.join(ROOT, 'include', 'cosmo_pol_amd.h')).read()
    declared = set(re.findall(r'CPOL_API\s+[\w \*]+?\b(cpol_\w+)\s*\(', header))
    assert declared == set(BEFORE) | set(NEW), sorted(declared ^ (set(BEFORE) | set(NEW)))


def _member(seed=0, shape=(5, 4, 6), names=('U', 'V', 'T')):
    rng = np.random.default_rng(seed)
    z = np.sort(rng.uniform(0, 1e4, shape).astype(np.float32), axis=0)[::-1].copy()
    return {'data': {k: rng.normal(size=shape).astype(np.float32) for k in names}, 'zlevels': z,
            'proj_info': {'Lo1': -1.0, 'La1': -2.0, 'Lo2': 1.0, 'La2': 2.0, 'Latitude_of_southern_pole': -43.0,
                          'Longitude_of_southern_pole': 10.0},
            'resolution': (0.02, 0.02)}


def test_check_members_names_the_member_and_what_differs():
    from cosmo_pol_amd import ensemble
    a = _member(0)

    def like_a(seed):
        m = _member(seed)
        m['zlevels'] = a['zlevels'].copy()
        return m
    ensemble.check_members([a, like_a(1), like_a(2)])           # same model, other states
    with pytest.raises(ValueError, match=r'at least two members'):
        ensemble.check_members([a])
    bad = like_a(3)
    bad['data'] = {k: v[:, :, :5].copy() for k, v in bad['data'].items()}
    with pytest.raises(ValueError, match=r'member 2: variable \w+ has shape \(5, 4, 5\)'):
        ensemble.check_members([a, like_a(1), bad])
    bad = like_a(4)
    bad['data']['QR_v'] = bad['data']['U'].copy()
    with pytest.raises(ValueError, match=r'member 1: variable set differs from member 0 \(QR_v\)'):
        ensemble.check_members([a, bad])
    bad = like_a(5)
    bad['zlevels'][2, 1, 3] += np.float32(0.5)
    with pytest.raises(ValueError, match=r'member 1: z-levels differ from member 0 in 1 value'):
        ensemble.check_members([a, bad])
    bad = like_a(6)
    bad['proj_info'] = dict(a['proj_info'], Lo1=-1.5)
    with pytest.raises(ValueError, match=r"member 1: grid differs from member 0 \(proj_info\['Lo1'\]"):
        ensemble.check_members([a, bad])
    bad = like_a(7)
    bad['resolution'] = (0.02, 0.03)
    with pytest.raises(ValueError, match=r'member 1: grid resolution'):
        ensemble.check_members([a, bad])


def test_chunk_planner():
    from cosmo_pol_amd import ensemble
    rng = np.random.default_rng(11)
    for _ in range(300):
        n = int(rng.integers(1, 90))
        members = list(rng.permutation(200)[:n])
        per = int(rng.integers(1, 10 ** 6))
        budget = int(rng.integers(0, 40 * 10 ** 6))
        cap = int(rng.integers(1, 70))
        chunks = ensemble.plan_member_chunks(members, per, budget, cap)
        assert [m for c in chunks for m in c] == members           # every member once, order kept
        assert all(1 <= len(c) <= cap for c in chunks)
        if budget >= per:                                          # the budget is honoured whenever one member fits
            assert all(len(c) * per <= budget for c in chunks)
        else:
            assert all(len(c) == 1 for c in chunks)
    assert ensemble.plan_member_chunks(range(5), 10, 10 ** 9) == [[0, 1, 2, 3, 4]]
    assert len(ensemble.plan_member_chunks(range(130), 1, 10 ** 9)) == 3      # 64 members per call
    assert ensemble.plan_member_chunks([], 10, 100) == []


def test_form_rule():
    from cosmo_pol_amd import ensemble
    assert ensemble.choose_form(1, 4) == 'per_member' and ensemble.choose_form(3, 4) == 'per_member'
    assert ensemble.choose_form(4, 4) == 'shared' and ensemble.choose_form(49, 4) == 'shared'
