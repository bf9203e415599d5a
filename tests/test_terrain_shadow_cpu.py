"""Terrain shadowing on the host: the rule in NumPy (cosmo_pol_amd/shadow.py) on hand-written rows, the two configuration keys,
the launch rule (cpol_forms.h: FormIn.shadow, through tests/c_host/shadow_forms_check.cpp) and the layout of the two structs that
carry the feature.  No expected value here comes from the code under test: the rows and their answers are written out."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import config as cfg
from cosmo_pol_amd import shadow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#          codes                         first  shadowed codes
ROWS = [([0, 0, 1, 0, 0, 1],             6,     [0, 0, 1, 0, 0, 1]),              # no hit: nothing moves
        ([-1, 0, 0, 1, 0, 0],            0,     [-1, -1, -1, -1, -1, -1]),         # hit at 0
        ([0, 1, 0, 0, 0, -1],            5,     [0, 1, 0, 0, 0, -1]),              # hit at the last gate
        ([1, 0, -1, 1, 0, 1],            2,     [1, 0, -1, -1, -1, -1]),           # +1 before and behind the hit: the one behind becomes -1
        ([0, -1, 0, -1, -1, 0],          1,     [0, -1, -1, -1, -1, -1]),          # several hits: the first decides
        ([0, 0, 2, -1, 2, 0],            3,     [0, 0, 2, -1, -1, -1])]            # outside the domain (2) before and behind the hit


def test_first_hit_and_apply_on_hand_written_rows():
    mask = np.array([r[0] for r in ROWS], dtype=np.int8)
    assert shadow.first_hit(mask).tolist() == [r[1] for r in ROWS]
    assert shadow.first_hit(mask[None]).shape == (1, len(ROWS))
    vals = np.arange(2 * mask.size, dtype=np.float32).reshape((2,) + mask.shape) + 1
    vals[0, 3, 4] = -9999.0
    vals[1, 4, 0] = np.nan                                 # a NaN in front of the hit stays what it is
    m2, v2 = shadow.apply_arrays(mask, vals)
    assert m2.dtype == np.int8 and v2.dtype == np.float32
    assert m2.tolist() == [r[2] for r in ROWS]
    for i, (_, first, _) in enumerate(ROWS):
        assert np.isnan(v2[:, i, first:]).all(), i
        assert v2[:, i, :first].tobytes() == vals[:, i, :first].tobytes(), i
    assert mask.tolist() == [r[0] for r in ROWS]           # the inputs are not written
    # idempotent
    m3, v3 = shadow.apply_arrays(m2, v2)
    assert m3.tobytes() == m2.tobytes() and v3.tobytes() == v2.tobytes()


def test_apply_on_a_columns_dict():
    mask = np.array([[r[0] for r in ROWS[:3]], [r[0] for r in ROWS[3:]]], dtype=np.int8)         # [2 rays, 3 sub-beams, 6 gates]
    rng = np.random.default_rng(1)
    cols = {'mask': mask, 'T': rng.random(mask.shape).astype(np.float32), 'QR_v': rng.random(mask.shape).astype(np.float32)}
    for k in shadow.GEOMETRY:
        cols[k] = rng.random(mask.shape).astype(np.float64 if k in ('lats', 'lons') else np.float32)
    cols['quad_pts'] = rng.random((2, 3, 2))
    cols['quad_weights'] = np.array([0.25, 0.5, 0.25])
    before = {k: np.array(v) for k, v in cols.items()}
    out = shadow.apply(cols)
    assert set(out) == set(cols)
    assert out['mask'].reshape(6, 6).tolist() == [r[2] for r in ROWS]
    hit = np.array([[g >= r[1] for g in range(6)] for r in ROWS]).reshape(mask.shape)
    for k in ('T', 'QR_v'):
        assert out[k].dtype == np.float32 and np.isnan(out[k][hit]).all() and np.array_equal(out[k][~hit], before[k][~hit]), k
    for k in shadow.GEOMETRY + ('quad_pts', 'quad_weights'):           # the geometry is never touched
        assert out[k] is cols[k], k
    for k, v in before.items():                                        # nor are the inputs
        assert np.array_equal(cols[k], v, equal_nan=True), k
    again = shadow.apply(out)
    for k in ('mask', 'T', 'QR_v'):
        assert np.array_equal(again[k], out[k], equal_nan=True), k
    with pytest.raises(ValueError):
        shadow.apply({k: v for k, v in cols.items() if k != 'mask'})
    with pytest.raises(ValueError):
        shadow.apply(dict(cols, QmS_v=cols['T']))                      # melted columns: the step belongs in front of the melting scheme
    with pytest.raises(ValueError):
        shadow.apply(dict(cols, T=cols['T'][:, :, :-1]))


def test_visibility_on_hand_written_rows():
    w = np.array([0.1, 0.7, 0.2])
    mask = np.zeros((3, 3, 4), dtype=np.int8)
    mask[0, :, 1] = -1                                     # ray 0, gate 1: every sub-beam blocked
    mask[1, 0, 2] = -1                                     # ray 1, gate 2: the first sub-beam blocked
    mask[1, 2, 3] = -1                                     # ray 1, gate 3: the last
    mask[2, 1, 0] = 1                                      # +1 and 2 are not blocked
    mask[2, 2, 0] = 2
    vis = shadow.visibility(mask, w)
    total = (np.float64(0.0) + 0.1 + 0.7) + 0.2
    assert vis.dtype == np.float64 and vis.shape == (3, 4)
    assert vis[0, 1] == 0.0 and not np.signbit(vis[0, 1])
    assert vis[1, 2] == ((np.float64(0.0) + 0.7) + 0.2) / total
    assert vis[1, 3] == ((np.float64(0.0) + 0.1) + 0.7) / total
    want_one = np.ones((3, 4), dtype=bool)
    want_one[0, 1] = want_one[1, 2] = want_one[1, 3] = False
    assert (vis[want_one] == 1.0).all()
    # the shadowed codes: everything behind a full block is 0.0
    vis_s = shadow.visibility(shadow.apply_arrays(mask, np.zeros((1,) + mask.shape, np.float32))[0], w)
    assert (vis_s[0, 1:] == 0.0).all() and vis_s[0, 0] == 1.0
    assert vis_s[1, 3] == (np.float64(0.0) + 0.7) / total   # both outer sub-beams now blocked there
    with pytest.raises(ValueError):
        shadow.visibility(mask, np.ones(mask.shape))       # per-gate weights (integration scheme 'ml'): refused
    with pytest.raises(ValueError):
        shadow.visibility(mask[0], w)


def _conf(**integration):
    return {'radar': {'coords': [46.5, 7.5, 1000], 'frequency': 5.6, '3dB_beamwidth': 1., 'K_squared': 0.93, 'range': 30000,
                      'radial_resolution': 300, 'sensitivity': [-5, 10000]}, 'integration': dict(integration)}


def test_config_keys_are_validated_and_stay_out_of_the_reference_tables():
    for key in ('terrain_shadow', 'terrain_visibility'):
        assert key not in cfg.DEFAULTS['integration'] and key not in cfg.VALID_VALUES['integration']
        assert key not in cfg.sanity_check(_conf())['integration']              # absent stays absent: off
        for ok in (0, 1, True, False):
            assert cfg.sanity_check(_conf(**{key: ok}))['integration'][key] == ok
        for bad in (2, -1, 'yes', 1.0, [1]):
            with pytest.raises(ValueError):
                cfg.sanity_check(_conf(**{key: bad}))


def test_launch_rule_on_the_host(tmp_path):
    exe = str(tmp_path / 'shadow_forms_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'c_host', 'shadow_forms_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tag, n, lost = r.stdout.split()
    assert tag == 'SHADOW_FORMS_OK' and int(n) > 10000 and int(lost) > 100         # (not vacuous: the shadow did take forms away)


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of the two structs as gcc sees the header == the ctypes mirrors; terrain_shadow took the slot of the
    former padding (nothing of cpol_sweep_params moved, a zero-initialised struct means off), visibility stands with the other
    per-geometry-row arrays behind heights."""
    pairs = [('cpol_sweep_params', N.SweepParams), ('cpol_outputs', N.Outputs)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "cosmo_pol_amd.h"', 'int main(void){']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['cpol_sweep_params p; cpol_outputs o; memset(&p, 0, sizeof p); memset(&o, 0, sizeof o);',
              'printf("zero %d\\n", p.terrain_shadow == 0 && o.visibility == NULL);',
              'printf("size_shadow %zu\\n", sizeof p.terrain_shadow);', 'return 0;}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert got['zero'] == '1' and got['size_shadow'] == '4'
    P, O = N.SweepParams, N.Outputs
    assert P.terrain_shadow.offset == P.var_edr.offset + 4 and P.sigma_r.offset == P.terrain_shadow.offset + 4
    assert P.v_res.offset + 8 == ctypes.sizeof(P)
    assert N.SweepParams().terrain_shadow == 0 and not N.Outputs().visibility
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert O.visibility.offset == O.heights.offset + ptr and O.model_vars.offset == O.visibility.offset + ptr
    assert not [n for n in N.EXPORTS if 'shadow' in n]      # (the kernel's test hook is a control name of cpol_debug_read: no new export)


def test_header_and_module_state_the_same_rule():
    with open(os.path.join(ROOT, 'include', 'cosmo_pol_amd.h')) as f:
        h = f.read()
    doc = h[h.index('/* Terrain shadowing ('):h.index('} cpol_outputs;')]
    for text in ('first = min{ g : c[g] == -1 }', 'For every g >= first', 'Gates g < first keep their bits', 'VISIBILITY', 'CPOL_ERR_ARG',
                 'cpol_run_columns', 'spaceborne'):
        assert text in doc, text
    for text in ('first = min{ g : c[g] == -1 }', 'for every g >= first', 'gates g < first keep their bits', 'VISIBILITY'):
        assert text in shadow.__doc__, text
    assert '"terrain_shadow_rows" is a CONTROL name' in h
