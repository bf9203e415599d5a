"""The scenarios of tests/_buckets.py hold the properties they are named for -- judged from the columns alone, with the oracle's
bin_index -- and the oracle gives finite scattering sums wherever they hold an item.  This is the guard against a scenario that
silently stops exercising its branch of the counting sort; tests/test_gpu_buckets.py pins the device on the same columns."""
import numpy as np
import pytest

import _buckets as B
import _cases
from cosmo_pol_oracle import scatter


def _counts_by_bucket(scn, model):
    """{(species, eb, tb): items} of the populated keys, from the host model."""
    _, n_t, base = B.key_layout(scn.case)
    out = {}
    for k in np.nonzero(model['hist'])[0]:
        j = max(q for q in range(len(scn.species)) if base[q] <= k)
        eb, tb = divmod(int(k) - base[j], n_t[j])
        out[(scn.species[j], eb, tb)] = int(model['hist'][k])
    return out


@pytest.mark.parametrize('name', B.SCENARIOS + ('sparse_blocks_previous',))
def test_keys_are_the_designed_ones_and_the_oracle_is_finite(name):
    scn = B.scenario(name)
    model = B.host_model(scn)
    assert np.array_equal(model['keys'], scn.design), 'a bin centre fell into another bin'
    assert scn.n_sub == 3 and scn.n_gates == 100 and (scn.n_sub * scn.n_gates) % B.CLASSIFY_THREADS != 0
    n_items = 0
    olut = {h: _cases.as_oracle_lut(l) for h, l in scn.luts.items()}
    present = (model['keys'] >= 0).reshape(len(scn.species), scn.n_rays, scn.n_sub, scn.n_gates)
    has_item = present.any(axis=(0, 2))
    # Doppler scheme 1 hands the fall-speed sums of ALL ice items of a sub-beam to its first gate with ice (IceParticle.integrate_V
    # returns one number): a gate whose only items are ice crystals has no radial velocity in the reference
    not_ice = [j for j, h in enumerate(scn.species) if h != 'I' or scn.conf['doppler']['scheme'] == 2]
    has_speed = present[not_ice].any(axis=(0, 2))
    if name == 'sparse_blocks_previous':
        # intended otherwise: rain of 1e-22 kg m-3 (beyond the integral tables, which is its purpose) leaves sums that are zero
        # in float32, and the reference turns exact zeros into NaN
        has_item = has_speed = np.zeros_like(has_item)
    for ray in range(scn.n_rays):
        o = scatter.radar_observables(scn.subbeams(ray), olut, scn.conf, return_sz=True)
        assert np.array_equal(np.isfinite(o.sz_total).all(axis=1), has_item[ray]), (name, ray)
        assert np.array_equal(np.isfinite(o.values['ZH']), has_item[ray]), (name, ray)
        assert np.isfinite(o.values['RVEL'][has_speed[ray]]).all(), (name, ray)
        n_items += int(np.isfinite(o.sz_integ[:, :, 0]).sum())
    assert model['n_valid'] <= 10000, 'the oracle work of one test stays below 10 000 items'
    assert (n_items == 0) == (name == 'empty') and (model['n_valid'] == 0) == (name == 'empty')


def test_item_reference_is_the_oracle_before_its_float32_store():
    """One sub-beam alone with weight w: sz_integ == float32(item_reference * w) exactly."""
    scn = B.scenario('species_borders_1mom')
    ref = B.item_reference(scn).reshape(len(scn.species), scn.n_rays, scn.n_sub, scn.n_gates, 12)
    olut = {h: _cases.as_oracle_lut(l) for h, l in scn.luts.items()}
    for ray, s in ((0, 0), (1, 2)):
        sb = scn.subbeams(ray)[s]
        o = scatter.radar_observables([sb], olut, scn.conf, return_sz=True)
        want = (ref[:, ray, s] * float(scn.cols['quad_weights'][s])).astype(np.float32).transpose(1, 0, 2)
        assert np.array_equal(o.sz_integ, want, equal_nan=True)
        assert np.isfinite(want).sum() > 12 * 50


@pytest.mark.parametrize('name', ['overflow_R', 'overflow_mS', 'overflow_two_species'])
def test_overflow_scenarios_fill_the_rank_tables(name):
    scn = B.scenario(name)
    keys = B.host_model(scn)['keys']
    a0, a1 = scn.notes['stretch_a']
    b0, b1 = scn.notes['stretch_b']
    assert a1 - a0 >= 3 * B.CLASSIFY_THREADS and a1 == b0
    for h in scn.notes['named']:
        kj = keys[scn.species.index(h)]
        # any 192 consecutive slots of stretch A: more distinct keys than the rank table has slots, and repeats beside them
        d = B.distinct_per_window(kj, a0, a1)
        assert d.min() > B.RANK_SLOTS, (h, d.min())
        assert (B.WINDOW - d).min() >= 40, 'no repeated keys inside the window'
        # any workgroup-sized window of stretch B fits into the table; together they hold every key of the walk
        d = B.distinct_per_window(kj, b0, b1, width=B.CLASSIFY_THREADS)
        assert d.max() <= B.RANK_SLOTS // 2 + 1, (h, d.max())
        walked = set(kj[a0:a1].tolist())
        assert walked == set(kj[b0:b1].tolist()) and len(walked) == scn.notes['n_walk'] > B.RANK_SLOTS
        # twins: the same (key, palette entry) -- identical inputs -- in stretch A and in stretch B
        pj = scn.palette[scn.species.index(h)]
        twins = set(zip(kj[a0:a1].tolist(), pj[a0:a1].tolist())) & set(zip(kj[b0:b1].tolist(), pj[b0:b1].tolist()))
        assert len(twins) >= scn.notes['n_walk']
    others = [j for j, h in enumerate(scn.species) if h not in scn.notes['named']]
    assert not (keys[others] >= 0).any()


@pytest.mark.parametrize('name', ['unit_edges_1mom', 'unit_edges_2mom', 'species_borders_1mom', 'species_borders_2mom',
                                  'scan_borders_per1', 'scan_borders_per3', 'ice_mixed_unit'])
def test_bucket_sizes_are_exact_and_spread(name):
    scn = B.scenario(name)
    model = B.host_model(scn)
    assert _counts_by_bucket(scn, model) == scn.notes['buckets']
    _, n_t, base = B.key_layout(scn.case)
    if name.startswith('unit_edges'):
        for h in scn.species:
            assert sorted(c for (hh, _, _), c in scn.notes['buckets'].items() if hh == h) == list(B.EDGE_COUNTS), h
    if name.startswith('species_borders'):
        populated = set(np.nonzero(model['hist'])[0].tolist())
        assert populated == set(base[:-1]) | set(b - 1 for b in base[1:])
        for j in range(len(scn.species)):
            assert model['hist'][base[j]] == 65 and model['hist'][base[j + 1] - 1] == 129
    if name.startswith('scan_borders'):
        per, want = B.scan_border_keys(base[-1])
        assert per == {'scan_borders_per1': 1, 'scan_borders_per3': 3}[name]
        assert np.nonzero(model['hist'])[0].tolist() == want
        assert {0, base[-1] - 1, per - 1, per, 512 * per - 1, 512 * per} <= set(want)
        assert all(k in want for k in (1023 * per - 1, 1023 * per) if k < base[-1])
    # the items of a bucket of 63 or more: in several classify workgroups and several rays, every palette entry among them
    for k in np.nonzero(model['hist'] >= 63)[0]:
        j = max(q for q in range(len(scn.species)) if base[q] <= k)
        slots = np.where(model['keys'][j] == k)[0]
        assert len(np.unique(slots // B.CLASSIFY_THREADS)) >= min(3, scn.n_sbg // B.CLASSIFY_THREADS), k
        assert len(np.unique(slots // (scn.n_sub * scn.n_gates))) >= 2 or scn.n_rays == 1, k
        assert set(scn.palette[j, slots].tolist()) >= set(range(B.PALETTE)), k


def test_unit_sizes_differ_between_neighbouring_species_somewhere():
    """species_borders needs neighbours with different unit sizes to see a key_base comparison that is off by one: the 2-moment
    configuration has them on three of its four borders (the 1-moment species all keep two items per lane)."""
    assert B.unit_shifts('c3_melt_ice') == (7, 7, 7, 7, 7, 7) and B.unit_shifts('c3_dop2') == (7,) * 6
    assert B.unit_shifts('c2_rsg') == (7, 7, 7)
    assert B.unit_shifts('c5_2mom') == (7, 6, 6, 7, 6)
    scn = B.scenario('species_borders_2mom')
    model = B.host_model(scn)
    # 65 and 129 items: ceil(c / 64) = 2, 3 against ceil(c / 128) = 1, 2 -- a wrong shift at a border changes the unit total
    assert model['n_units'] == sum((2 + 3) if s == 6 else (1 + 2) for s in model['shifts'])


def test_many_units_outnumber_every_persistent_grid():
    scn = B.scenario('many_units')
    model = B.host_model(scn)
    assert (model['hist'] >= 1).all() and len(model['hist']) == 2752
    assert model['n_units'] == 2752 > 1024
    assert len(scn.species) == 6


def test_sparse_blocks_leave_whole_workgroups_without_melting_items():
    scn, prev = B.scenario('sparse_blocks'), B.scenario('sparse_blocks_previous')
    keys = B.host_model(scn)['keys']
    melting = [scn.species.index(h) for h in B.MELTING]
    ranked = np.where((keys[melting] >= 0).any(axis=0))[0]
    assert ranked.tolist() == list(scn.notes['ranked_slots'])
    blocks = set((ranked // B.CLASSIFY_THREADS).tolist())
    n_blocks = -(-scn.n_sbg // B.CLASSIFY_THREADS)
    assert scn.n_sbg % B.CLASSIFY_THREADS != 0 and len(blocks) >= 3 and n_blocks - len(blocks) >= 4
    r = scn.species.index('R')
    assert (keys[r] >= 0).all(), 'rain in every slot: the skipped workgroups hold tabulated items'
    # the call before it ranks rain in those very gates, and nothing else
    pk = B.host_model(prev)['keys']
    assert prev.n_sbg == scn.n_sbg and (pk[r] >= 0).all() and not (np.delete(pk, r, axis=0) >= 0).any()
    assert 0 < prev.flat('QR_v').min() and prev.flat('QR_v').max() < 1e-21


def test_ice_mixed_unit_has_exactly_one_lambda_outside_the_tables():
    from cosmo_pol_amd import hydrometeors as H
    scn = B.scenario('ice_mixed_unit')
    model = B.host_model(scn)
    i = scn.species.index('I')
    _, n_t, base = B.key_layout(scn.case)
    for key, n_out in ((B.ICE_MIXED_KEY, 1), (B.ICE_PLAIN_KEY, 0)):
        slots = np.where(model['keys'][i] == base[i] + key[0] * n_t[i] + key[1])[0]
        assert len(slots) == 64
        l2 = np.array([B.ice_log2_lambda(scn.flat('T')[s], scn.flat('QI_v')[s])[0] for s in slots])
        outside = ~((l2 >= H.ICE_LOG2_LO) & (l2 < H.ICE_LOG2_HI))
        assert outside.sum() == n_out, l2
        if n_out:
            assert slots[outside][0] == scn.notes['odd_slot'] and l2[outside][0] > H.ICE_LOG2_HI + 0.5
    assert B.unit_shifts(scn.case)[i] == 7 and model['n_units'] == 2


def test_empty_and_one_item():
    e, o = B.scenario('empty'), B.scenario('one_item')
    assert B.host_model(e)['n_valid'] == 0 and B.host_model(e)['n_units'] == 0
    m = B.host_model(o)
    assert m['n_valid'] == 1 and m['n_units'] == 1
    assert np.argwhere(m['keys'] >= 0).tolist() == [[o.species.index('S'), o.n_sbg - 1]]


def test_doppler_schemes_and_scan_regimes_are_covered():
    schemes = {n: B.scenario(n).conf['doppler']['scheme'] for n in B.SCENARIOS}
    assert 1 in schemes.values() and 2 in schemes.values(), schemes
    assert schemes['unit_edges_1mom'] == 2 and schemes['overflow_mS'] == 2
    assert B.key_layout('c2_rsg')[2][-1] == 840 and B.key_layout('c3_melt_ice')[2][-1] == 2752
    for name in B.STALE_SEQUENCE:
        assert B.scenario(name, 'c3_melt_ice').species == B.scenario('many_units').species


def test_solo_copies_one_item():
    scn = B.scenario('unit_edges_2mom')
    model = B.host_model(scn)
    j = scn.species.index('G')
    slot = int(np.where(model['keys'][j] >= 0)[0][0])
    cols, at = B.solo(scn, slot, j)
    assert cols['elev'].shape == (1, 3, 100) and at == 299
    for k in ('T', 'elev', 'QG_v', 'QNG_v'):
        assert cols[k].reshape(-1)[at] == scn.flat(k)[slot]
    assert sum(int((cols[k] > 0).sum()) for k in cols if k.startswith('Q') and not k.startswith('QN')) == 1
