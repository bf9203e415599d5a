"""The counting sort and its work units at every bucket shape (tests/_buckets.py), on the device.

A sweep integrates an item bin by bin whenever its slot has no integral table: k_classify ranks the item in its LDS rank tables,
k_bucket_scan scans the bucket counts, k_bucket_scatter writes perm[] and the unit list, the integrating kernels walk the units.
The interpolated radials of the other modules never fill a rank table, never stride a persistent grid and leave the bucket sizes
to chance; the scenarios here are built so that each such branch MUST be taken, and the equalities of form A are what shows
that it was: every item's key, the histogram, the item count and the unit count equal a host model made from the columns alone.

  form A  CPOL_ITAB=0: every item goes through the sort.  Keys, histogram and counters against the host model; every item's
          float64 result (item_res) at 1e-5 relative against the same item recomputed from the oracle's own parts before its
          float32 store; items with identical inputs -- planted in the first and second slot of a lane, in different units of a
          bucket, in a unit of 1 beside units of 128, in different classify workgroups, behind a slot ticket and behind a direct
          claim -- give identical bits; the first item of every unit_edges bucket gives the same bits when it is alone in a call;
          sz_integ, sz_total and ZH ... RVEL against scatter.radar_observables at the tolerances of tests/test_gpu_parity.py
          (1e-5 relative, the operand-scaled atol of KDP / PHIDP / DELTA_HV, 2e-4 m/s for RVEL), NaN patterns and masks equal;
          the call without the debug reads gives the same bits.
  form B  the integral tables on: the chain stays idle (no work unit, every item on a table) and the outputs agree with the
          oracle at the same tolerances and with form A in their NaN patterns (what tests/test_gpu_bad_values.py asks of its
          no_integral_tables form).
  form C  CPOL_ITAB_MELT=0: the melting species are sorted, the others sit on tables; sparse_blocks after a call that ranked
          rain in every gate: pos[] of the workgroups that rank nothing now still holds that call's positions, and is not read.
  stale   many_units, one_item, empty, unit_edges on one operator: the bits of a fresh operator each.

(1-moment ice: a group of identical items whose units differ in whether they pass ice_unit_in_table -- k_psd_ice2 reads the
normalisation from its tables, k_psd<ICE> sums it -- may differ in the last bits.  No scenario plants such a group: the items of
a palette entry share their bucket, and ice_mixed_unit's buckets are one unit each; its odd item is compared with the reference
like every other.)

Tried against scratch builds with one edit each (cpol_psd.inl); each leaves wrong numbers, none an index out of bounds:
  * unit_shift_of comparing `k > key_base[q]`: form A of species_borders_2mom fails at n_work_units (20 against 21);
    species_borders_1mom, whose species all share one unit size, and unit_edges_2mom, whose buckets lie inside the species, pass;
  * thread 1023 of k_bucket_scan writing totals[1] = ubase - 1: form A of one_item (0 units against 1) and scan_borders_per1 (6
    against 7) fail at n_work_units; empty passes;
  * k_bucket_scatter without the blk_ranked skip: form C of sparse_blocks fails against the oracle (RVEL of ray 0, where the
    stale positions of the call before overwrote perm[] of a melting item); form A and form B of sparse_blocks pass.
Not run: rank_position dropping the direct claims.  Its unplaced items leave entries of perm[] unwritten, and the integrating
kernels would use whatever those hold as gate indices -- that is no build for a GPU.  By the code, such a build leaves the rows
of item_res of every directly claimed item unwritten: form A of the three overflow scenarios compares each of them."""
import numpy as np
import pytest

import _buckets as B
import _cases
from cosmo_pol_oracle import scatter

pytestmark = pytest.mark.gpu

RTOL = 1e-5
KNOBS = ('CPOL_ITAB', 'CPOL_ITAB_MELT', 'CPOL_ITAB_MAX_DEV', 'CPOL_ITAB_KEEP_PANELS', 'CPOL_RARE_DIRECT', 'CPOL_GATE1', 'CPOL_SUBSUM',
         'CPOL_PSD_RARE', 'CPOL_ICE_FORCE_SUM', 'CPOL_FUSE_CLASSIFY', 'CPOL_USE_GRAPH')
FORM_ENV = {'A': {'CPOL_ITAB': '0'}, 'B': {}, 'C': {'CPOL_ITAB_MELT': '0'}}
POL = ['ZH', 'ZV', 'ZDR', 'RHOHV', 'KDP', 'ATT_H', 'ATT_V', 'DELTA_HV', 'PHIDP']
PUBLIC = POL + ['RVEL', 'mask']


def _operator(monkeypatch, form, scn):
    """The knobs are read when the context is created and when the tables are built: they stay set until the test ends."""
    from cosmo_pol_amd import RadarOperator
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORM_ENV[form].items():
        monkeypatch.setenv(k, v)
    return RadarOperator(config=scn.over, luts=scn.luts, output_variables='only_radar')


def _run(op, scn, debug=True, cols=None, items=True):
    op._ctx.enable_debug(debug)
    res = op.simulate_columns(dict(scn.cols if cols is None else cols))
    n_rays = 1 if cols is not None else scn.n_rays
    assert res['n_sub'] == scn.n_sub and res['ZH'].shape == (n_rays, scn.n_gates)
    out = {k: res[k] for k in PUBLIC}
    if debug:
        nh, n_sbg = len(scn.species), n_rays * scn.n_sub * scn.n_gates
        ctx = op._ctx
        out['item_key'] = ctx.debug_read('item_key', (nh, n_sbg), np.int32)
        out['bucket_count'] = ctx.debug_read('bucket_count', (B.key_layout(scn.case)[2][-1],), np.int32)
        if items:
            out['item_res'] = ctx.debug_read('item_res', (nh, n_sbg, 12), np.float64)
        out['sz_integ'] = ctx.debug_read('sz_integ', (n_rays, scn.n_gates, nh, 12), np.float32)
        out['sz_total'] = ctx.debug_read('sz_total', (n_rays, scn.n_gates, 12), np.float32)
        c = ctx.counters()
        out['counters'] = dict(n_valid_items=int(c.n_valid_items), n_table_items=int(c.n_table_items),
                               n_work_units=int(c.n_work_units), n_subbeam_gates=int(c.n_subbeam_gates))
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(u), b[~nb].view(u))


def _assert_same_public(got, ref, tag, keys=PUBLIC):
    for k in keys:
        assert _same(got[k], ref[k]), '%s: %s differs' % (tag, k)


def _tol(k, sz, conf):
    """tests/test_gpu_parity.py::_pol_tolerances."""
    from cosmo_pol_oracle import constants as OK
    wl = OK.Derived(conf).WAVELENGTH
    res_km = conf['radar']['radial_resolution'] / 1000.
    kdp = np.nan_to_num(1e-3 * (180.0 / np.pi) * wl * (np.abs(sz[:, 8]) + np.abs(sz[:, 10])))
    return {'KDP': RTOL * kdp, 'PHIDP': RTOL * (np.cumsum(2 * kdp) * res_km + np.pi), 'DELTA_HV': RTOL * np.pi}.get(k, 0.0)


_ORACLE = {}


def _oracle(scn):
    """The oracle's radials of a scenario, computed once and left unchanged."""
    if (scn.name, scn.case) not in _ORACLE:
        olut = {h: _cases.as_oracle_lut(l) for h, l in scn.luts.items()}
        _ORACLE[(scn.name, scn.case)] = [scatter.radar_observables(scn.subbeams(r), olut, scn.conf, return_sz=True) for r in range(scn.n_rays)]
    return _ORACLE[(scn.name, scn.case)]


def _against_oracle(out, scn, tag, sz=True):
    n = 0
    for r, o in enumerate(_oracle(scn)):
        t = '%s %s ray %d' % (tag, scn.name, r)
        if sz:
            _cases.assert_close_nan(out['sz_integ'][r], o.sz_integ, rtol=RTOL, name='sz_integ ' + t)
            _cases.assert_close_nan(out['sz_total'][r], o.sz_total, rtol=RTOL, name='sz_total ' + t)
        szt = np.nan_to_num(o.sz_total.astype(np.float64))
        for k in POL:
            _cases.assert_close_nan(out[k][r], o.values[k], rtol=RTOL, atol=_tol(k, szt, scn.conf), name='%s %s' % (k, t))
        _cases.assert_close_nan(out['RVEL'][r], o.values['RVEL'], rtol=RTOL, atol=2e-4, name='RVEL ' + t)
        assert np.array_equal(out['mask'][r], o.mask), t
        n += int(np.isfinite(o.values['ZH']).sum())
    return n


def _record(rec):
    """Printed and appended to bucket_records.jsonl beside the parity and rough-table records of the run."""
    from test_gpu_rough_tables import _record as write
    write(rec, name='bucket_records.jsonl', tag='BUCKETS')


def _assert_sorted_as_the_host_says(out, scn, model, n_table=0, tag='form A'):
    """Keys, histogram of the ranked items and counters of a call in which the species `ranked` went through the sort."""
    assert np.array_equal(out['item_key'], model['keys']), '%s %s: item_key' % (tag, scn.name)
    c = out['counters']
    assert c['n_subbeam_gates'] == scn.n_sbg
    assert c['n_valid_items'] == model['n_valid'], (tag, scn.name, c)
    assert c['n_table_items'] == n_table, (tag, scn.name, c)


def _twin_groups(scn, model):
    """-> [(species index, slots)] of the items with identical inputs: one bucket, one palette entry, two items or more."""
    groups = []
    for j in range(len(scn.species)):
        idx = np.where(model['keys'][j] >= 0)[0]
        ident = model['keys'][j, idx].astype(np.int64) * 16 + scn.palette[j, idx]
        order = np.argsort(ident, kind='stable')
        cut = np.where(np.diff(ident[order]) != 0)[0] + 1
        groups += [(j, idx[g]) for g in np.split(order, cut) if len(g) >= 2]
    return groups


def _device_summary(out, scn, model):
    """What the device itself reports, for the records: bucket sizes, the unit total and, for the overflow scenarios, the
    distinct keys per window of 192 and per classify workgroup, counted on the device's keys."""
    sizes, counts = np.unique(out['bucket_count'][out['bucket_count'] > 0], return_counts=True)
    rec = {'bucket_sizes': {int(s): int(n) for s, n in zip(sizes, counts)}, 'n_work_units': out['counters']['n_work_units'],
           'n_valid_items': out['counters']['n_valid_items']}
    if 'stretch_a' in scn.notes:
        a0, a1 = scn.notes['stretch_a']
        for h in scn.notes['named']:
            kj = out['item_key'][scn.species.index(h)]
            d = B.distinct_per_window(kj, a0, a1)
            blocks = [len(np.unique(kj[p:p + B.CLASSIFY_THREADS][kj[p:p + B.CLASSIFY_THREADS] >= 0]))
                      for p in range(0, scn.n_sbg, B.CLASSIFY_THREADS)]
            rec['distinct_keys_' + h] = {'per_window_192_min': int(d.min()), 'per_window_192_max': int(d.max()),
                                         'per_classify_workgroup': blocks}
            assert d.min() > B.RANK_SLOTS and max(blocks) > B.RANK_SLOTS
    return rec


@pytest.mark.parametrize('name', B.SCENARIOS)
def test_form_a_every_item_through_the_sort(monkeypatch, name):
    scn = B.scenario(name)
    model = B.host_model(scn)
    op = _operator(monkeypatch, 'A', scn)
    try:
        out = _run(op, scn)
        plain = _run(op, scn, debug=False)
        solos = []
        if name.startswith('unit_edges'):
            # the first item of every bucket alone in a call, at the last sub-beam gate
            _, n_t, base = B.key_layout(scn.case)
            for k in np.nonzero(model['hist'])[0]:
                j = max(q for q in range(len(scn.species)) if base[q] <= k)
                slot = int(np.where(model['keys'][j] == k)[0][0])
                cols, at = B.solo(scn, slot, j)
                alone = _run(op, scn, cols=cols)
                assert alone['counters']['n_valid_items'] == 1 and alone['counters']['n_work_units'] == 1, (name, k)
                assert alone['item_key'][j, at] == k
                solos.append((j, slot, int(model['hist'][k]), alone['item_res'][j, at].copy()))
    finally:
        op.close()
    # ---- the sort did what the host model says: this is what shows that the scenario's branch ran on the device ----
    _assert_sorted_as_the_host_says(out, scn, model)
    assert np.array_equal(out['bucket_count'].astype(np.int64), model['hist']), name
    assert out['counters']['n_work_units'] == model['n_units'], (name, out['counters'], model['n_units'])
    rec = {'scenario': name, 'case': scn.case, 'form': 'A', 'doppler_scheme': scn.conf['doppler']['scheme'],
           'shape': [scn.n_rays, scn.n_sub, scn.n_gates], 'unit_shifts': list(model['shifts'])}
    rec.update(_device_summary(out, scn, model))
    # ---- every item against its float64 recomputation ----
    ref = B.item_reference(scn)
    worst, where = {}, {}
    _, n_t, base = B.key_layout(scn.case)
    for j, h in enumerate(scn.species):
        v = np.where(model['keys'][j] >= 0)[0]
        if not len(v):
            continue
        got, want = out['item_res'][j, v], ref[j, v]
        assert np.isfinite(want).all() and (want != 0).all(), (name, h)
        dev = np.abs(got - want) / np.abs(want)
        dev = np.where(np.isnan(dev), np.inf, dev)
        worst[h] = float(dev.max())
        i, c = np.unravel_index(np.argmax(dev), dev.shape)
        eb, tb = divmod(int(model['keys'][j, v[i]]) - base[j], n_t[j])
        where[h] = '%d of %d items above 1e-5; worst: slot %d, elevation bin %d, second-axis bin %d, column %d: %r against %r' % (
            int((dev > RTOL).any(axis=1).sum()), len(v), int(v[i]), eb, tb, int(c), got[i, c], want[i, c])
    rec['item_res_worst_rel'] = worst
    # ---- an item is a function of itself ----
    groups = _twin_groups(scn, model)
    rec['twin_groups'] = len(groups)
    rec['twin_items'] = int(sum(len(s) for _, s in groups))
    _record(rec)
    for h, w in worst.items():
        assert w <= RTOL, '%s: item_res of %s deviates by %.3e from the float64 recomputation (%s)' % (name, h, w, where[h])
    for j, slots in groups:
        rows = out['item_res'][j, slots].view(np.uint64)
        assert (rows == rows[0]).all(), '%s: %s items with identical inputs differ (slots %s ...)' % (
            name, scn.species[j], slots[:6].tolist())
    if name not in ('empty', 'one_item', 'many_units'):           # (many_units: one item per key, no two alike)
        assert len(groups) >= 2, name
    for j, slot, count, row in solos:
        assert np.array_equal(row.view(np.uint64), out['item_res'][j, slot].view(np.uint64)), \
            '%s: the first %s item of a bucket of %d, alone in a call, gives other bits' % (name, scn.species[j], count)
    if name.startswith('unit_edges'):
        assert len(solos) == len(B.EDGE_COUNTS) * len(scn.species)
    # ---- against the reference ----
    n = _against_oracle(out, scn, 'form A')
    assert (n > 0) == (name != 'empty')
    if name == 'empty':
        assert all(np.isnan(out[k]).all() for k in POL)
    # ---- without the debug reads ----
    _assert_same_public(plain, out, name + ': debug reads off')


@pytest.mark.parametrize('name', B.SCENARIOS)
def test_form_b_the_chain_stays_idle_with_the_tables_on(monkeypatch, name):
    """The integral tables take every item (their lambda ranges cover Q_RANGE): no work unit.  ice_mixed_unit's odd item lies
    beyond the ice table as well and is the one item integrated."""
    scn = B.scenario(name)
    model = B.host_model(scn)
    n_off = 1 if name == 'ice_mixed_unit' else 0
    op = _operator(monkeypatch, 'B', scn)
    try:
        out = _run(op, scn, items=False)
    finally:
        op.close()
    _assert_sorted_as_the_host_says(out, scn, model, n_table=model['n_valid'] - n_off, tag='form B')
    assert out['counters']['n_work_units'] == n_off, (name, out['counters'])
    assert int(out['bucket_count'].sum()) == n_off
    _against_oracle(out, scn, 'form B')
    op = _operator(monkeypatch, 'A', scn)
    try:
        a = _run(op, scn, debug=False)
    finally:
        op.close()
    for k in PUBLIC:
        assert np.array_equal(np.isnan(a[k]), np.isnan(out[k])), (name, k)
    assert np.array_equal(a['mask'], out['mask'])


@pytest.mark.parametrize('name', B.MELTING_SCENARIOS)
def test_form_c_sorts_the_melting_species_alone(monkeypatch, name):
    """CPOL_ITAB_MELT=0.  sparse_blocks: the call before it on the same context ranks rain in every gate (sparse_blocks_previous), so
    pos[] of the four classify workgroups that rank nothing in sparse_blocks still holds positions >= 0 of rain items -- which are
    present there again, now on their table.  k_bucket_scatter must skip those workgroups (blk_ranked): without the skip it
    scatters their gates into perm[] over the melting items' entries (a scratch build without the skip fails here)."""
    scn = B.scenario(name)
    model = B.host_model(scn)
    _, _, base = B.key_layout(scn.case)
    melting = [scn.species.index(h) for h in B.MELTING]
    ranked = np.zeros(len(model['hist']), dtype=np.int64)
    n_units = 0
    for j in melting:
        ranked[base[j]:base[j + 1]] = model['hist'][base[j]:base[j + 1]]
        n_units += int(np.sum(-(-model['hist'][base[j]:base[j + 1]] // (1 << model['shifts'][j]))))
    if name == 'ice_mixed_unit':                   # its odd item lies beyond the ice table too
        i = scn.species.index('I')
        ranked[model['keys'][i, scn.notes['odd_slot']]] += 1
        n_units += 1
    op = _operator(monkeypatch, 'C', scn)
    try:
        if name == 'sparse_blocks':
            prev = B.scenario('sparse_blocks_previous')
            before = _run(op, prev, items=False)
            assert before['counters']['n_table_items'] == 0 and before['counters']['n_valid_items'] == prev.n_sbg
            assert int(before['bucket_count'].sum()) == prev.n_sbg, 'the call before did not rank rain in every gate'
        out = _run(op, scn, items=False)
        plain = _run(op, scn, debug=False)
    finally:
        op.close()
    _assert_sorted_as_the_host_says(out, scn, model, n_table=model['n_valid'] - int(ranked.sum()), tag='form C')
    assert np.array_equal(out['bucket_count'].astype(np.int64), ranked), name
    assert out['counters']['n_work_units'] == n_units, (name, out['counters'], n_units)
    _against_oracle(out, scn, 'form C')
    _assert_same_public(plain, out, name + ': form C, debug reads off')
    _record({'scenario': name, 'case': scn.case, 'form': 'C', 'n_work_units': out['counters']['n_work_units'],
             'n_table_items': out['counters']['n_table_items'], 'n_valid_items': out['counters']['n_valid_items']})
    if name == 'sparse_blocks':
        op = _operator(monkeypatch, 'C', scn)
        try:
            fresh = _run(op, scn, items=False)
        finally:
            op.close()
        _assert_same_public(out, fresh, 'sparse_blocks after a call that ranked every gate', keys=PUBLIC + ['sz_integ', 'sz_total'])


def test_stale_state_of_the_previous_call(monkeypatch):
    """count[], pos[], perm[] and the unit list are reused from call to call: many units, then one item, then none, then the
    bucket edges on ONE operator -- each with the bits of a fresh operator."""
    scns = [B.scenario(n, 'c3_melt_ice') for n in B.STALE_SEQUENCE]
    keys = PUBLIC + ['sz_integ', 'sz_total', 'item_key', 'bucket_count']
    op = _operator(monkeypatch, 'A', scns[0])
    try:
        chain = [_run(op, s, items=False) for s in scns]
    finally:
        op.close()
    for s, got in zip(scns, chain):
        model = B.host_model(s)
        assert got['counters']['n_work_units'] == model['n_units'] and got['counters']['n_valid_items'] == model['n_valid'], s.name
        op = _operator(monkeypatch, 'A', s)
        try:
            fresh = _run(op, s, items=False)
        finally:
            op.close()
        _assert_same_public(got, fresh, 'after other calls: ' + s.name, keys=keys)
        assert got['counters'] == fresh['counters'], s.name
