"""The product object of the hydrometeor contributions (cosmo_pol_amd/species.py: Contributions) without an operator or a
device, as tests/test_products_cpu.py checks the others: the array list written out, every struct slot after `bind`, device
entries accepted and refused, `finish` and `join` on hand-made arrays."""
import ctypes as C

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import species as SP

f4, u1 = np.float32, np.uint8
AZ2 = np.arange(2.0)
SLOTS = ['R', 'S', 'G']


def attach(product, az, n_gates, n_members=None):
    structs, keep = product.attach(N, az, n_gates, n_members, True, False, ['U', 'V', 'W', 'T'], None)
    for slot in structs:
        assert slot in dict(N.Outputs._fields_)          # the slot of cpol_outputs its struct hangs on
    assert keep == []
    return structs


def test_struct_mirror_names_the_rules_fields_in_order():
    assert tuple(N.SPECIES_FIELDS) == SP.FIELDS
    names = [n for n, _ in N.Species._fields_]
    assert names == list(SP.FIELDS) + ['dominant', 'present', 'share', 'sz', 'n_hydro', 'pad_']
    assert C.sizeof(N.Species) == 12 * C.sizeof(C.c_void_p) + 8
    outs = [n for n, _ in N.Outputs._fields_]
    assert outs[outs.index('lats') - 1] == 'species' and outs[outs.index('species') - 1] == 'mask'
    assert outs[-2:] == ['member_stats', 'superob'] and outs[:-2] == N.OUTPUT_FIELDS
    assert SP.MAX_HYDRO == N.CPOL_MAX_HYDRO


def test_arrays_binding_finish_join():
    spec = SP.Species(fields=('KDP', 'ZH'), dominant=True, raw=True)
    p = SP.Contributions(spec, SLOTS, keep_gates=False)
    assert (p.name, p.gates, p.spectrum, p.model_var, p.names) == ('species', False, True, None, ('R', 'S', 'G'))
    assert SP.Contributions(spec, SLOTS).gates
    sp = attach(p, AZ2, 5)['species']
    assert isinstance(sp, N.Species) and sp.n_hydro == 3
    assert p.arrays() == [('ZH', f4, (3, 2, 5)), ('KDP', f4, (3, 2, 5)), ('dominant', u1, (2, 5)), ('present', u1, (2, 5)),
                          ('share', f4, (2, 5)), ('sz', f4, (2, 5, 3, 12))]
    bound = {}
    for i, (path, _, _) in enumerate(p.arrays()):
        bound[path] = 0x1000 * (i + 1)
        p.bind(path, bound[path])
    for name, _ in N.Species._fields_[:12]:               # every pointer slot: bound to its own address, or left NULL
        assert (getattr(sp, name) or 0) == bound.get(name, 0), name
    with pytest.raises(ValueError, match="no array 'PHIDP'"):
        p.bind('PHIDP', 1)

    fields_only = SP.Contributions(SP.Species(fields=('ZDR',), dominant=False), SLOTS)
    attach(fields_only, AZ2, 5)
    assert fields_only.arrays() == [('ZDR', f4, (3, 2, 5))]
    raw_only = SP.Contributions(SP.Species(fields=(), dominant=False, raw=True), ['R'])
    attach(raw_only, AZ2, 5)
    assert raw_only.arrays() == [('sz', f4, (2, 5, 1, 12))]

    w = {k: np.zeros(sh, dt) for k, dt, sh in p.arrays()}
    out = p.finish(dict(w), None)
    assert sorted(out) == ['KDP', 'ZH', 'dominant', 'names', 'present', 'share', 'sz'] and out['names'] == ('R', 'S', 'G')
    assert all(out[k] is w[k] for k in w)
    joined = p.join([out, out], np.concatenate)
    assert joined['names'] == ('R', 'S', 'G')
    assert joined['ZH'].shape == (3, 4, 5) and joined['dominant'].shape == (4, 5) and joined['sz'].shape == (4, 5, 3, 12)


def test_device_entries_accepted_and_refused():
    p = SP.Contributions(SP.Species(fields=('ZH',), dominant=True), SLOTS)
    sp = attach(p, AZ2, 5)['species']
    p.bind_device({'ZH': 11, 'share': 12, 'dominant': 13})
    assert (sp.ZH, sp.share, sp.dominant, sp.present or 0, sp.KDP or 0, sp.sz or 0) == (11, 12, 13, 0, 0, 0)
    with pytest.raises(ValueError, match="unknown entry 'KDP'"):
        p.bind_device({'KDP': 1})                          # (a field of the rule, but not of this spec)
    with pytest.raises(ValueError, match="unknown entry 'sz'"):
        p.bind_device({'sz': 1})
    with pytest.raises(ValueError, match="unknown entry 'moments'"):
        p.bind_device({'moments': 1})


def test_refusals():
    spec = SP.Species()
    with pytest.raises(ValueError, match='a cosmo_pol_amd.species.Species'):
        SP.Contributions(('ZH',), SLOTS)
    with pytest.raises(NotImplementedError, match='process group'):
        SP.Contributions(spec, SLOTS, distributed=True)
    with pytest.raises(ValueError, match='hydrometeor slots'):
        SP.Contributions(spec, [])
    with pytest.raises(NotImplementedError, match='no ensemble call'):
        attach(SP.Contributions(spec, SLOTS), AZ2, 5, n_members=2)
    assert set(SP.Contributions.refuses) == {'members', 'subbeams', 'groups'}      # (a time-blended call is taken)


def test_a_device_entry_of_the_operator_is_a_dict_under_the_products_name():
    # `species` is listed in no table of radar_operator.py: _run_rays takes a dict entry for the call's product by its name
    from cosmo_pol_amd.radar_operator import _PRODUCT_OUTPUTS
    assert SP.Contributions.name not in _PRODUCT_OUTPUTS and SP.Contributions.name in N.OUTPUT_FIELDS
