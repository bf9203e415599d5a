"""The per-radial seam without a GPU: the C ABI mirror of cpol_columns_t, the host-side integrate_radials /
combine_subradials against the oracle, and the argument checks that run before any device call."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _cases
from cosmo_pol_oracle import beam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seam_struct_layouts_match_header(tmp_path):
    from cosmo_pol_amd import _native as N
    pairs = [('cpol_columns_t', N.Columns), ('cpol_subbeam_outputs', N.SubbeamOutputs)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cosmo_pol_amd.h"', 'int main(void){']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert 'cpol_run_columns' in N.EXPORTS and 'cpol_interp_subbeams' in N.EXPORTS


def _oracle_subs(name):
    conf, az, el, ocube, luts, cube = _cases.radial_case(name)
    return conf, beam.interpolate_radial(ocube, conf, az, el)


@pytest.mark.parametrize('name', ['c2_rsg', 'c4_7x7', 'q_ml_thr'])
def test_integrate_radials_matches_oracle(name):
    from cosmo_pol_amd import radial
    _, subs = _oracle_subs(name)
    before = copy.deepcopy(subs)
    got = radial.integrate_radials(subs)
    ref = beam.integrate_subbeams(before)
    for k, v in ref.values.items():
        np.testing.assert_allclose(got.values[k], v, rtol=1e-12, err_msg=k)
    assert np.array_equal(got.mask, ref.mask)
    c = subs[int(len(subs) / 2)]
    assert got.dist_profile is c.dist_profile and got.lats_profile is c.lats_profile
    for a, b in zip(subs, before):                     # the records are not modified
        for k in b.values:
            assert np.array_equal(a.values[k], b.values[k], equal_nan=True)


def test_combine_subradials_reference_semantics():
    from cosmo_pol_amd import radial
    _, subs = _oracle_subs('c2_rsg')
    a = radial.Radial({'ZH': np.ones(3)}, np.zeros(3), None, None, np.arange(3.), None)
    b = radial.Radial({'RVEL': np.full(3, 2.0)}, np.zeros(3), None, None, np.arange(3.), None)
    out = radial.combine_subradials([a, b])
    assert out is a and set(out.values) == {'ZH', 'RVEL'}
    c = radial.Radial({'KDP': np.zeros(3)}, np.zeros(3), None, None, np.arange(3.) + 1, None)
    assert radial.combine_subradials([a, c]) is None
    # oracle sub-radials of one radial share their gates
    assert radial.combine_subradials(subs[:1] + subs[:1]) is subs[0]


def test_subradials_to_columns_checks():
    from cosmo_pol_amd import radial
    conf, subs = _oracle_subs('c4_7x7')
    names = list(subs[0].values)[:3]
    cols = radial.subradials_to_columns(subs, names, True)
    assert cols['elev'].shape == (1, len(subs), len(subs[0].mask))
    assert cols['QmS_v'].dtype == np.float32 and cols['fwet_mS'].dtype == np.float64
    ragged = copy.deepcopy(subs)
    ragged[1].mask = ragged[1].mask[:-1]
    with pytest.raises(ValueError):
        radial.subradials_to_columns(ragged, names, True)
    mixed = copy.deepcopy(subs)
    mixed[0].quad_weight = np.ones(len(mixed[0].mask))
    with pytest.raises(ValueError):
        radial.subradials_to_columns(mixed, names, True)
    with pytest.raises(ValueError):
        radial.subradials_to_columns(subs, names + ['NOT_A_VARIABLE'], True)
    with pytest.raises(ValueError):
        radial.subradials_to_columns([], names, True)
