"""The product objects a sweep call takes ("How a product plugs into a sweep call") and the block packer, on
their own: no operator, no library context -- only the ctypes structs of _native.  What can go wrong here is a slot index."""
import ctypes as C

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import ensemble_stats as ES
from cosmo_pol_amd import ensemble_verify as EV
from cosmo_pol_amd import histogram as HG
from cosmo_pol_amd import spectrum_moments as SM
from cosmo_pol_amd import superob as SO
from cosmo_pol_amd.radar_operator import _PRODUCT_OUTPUTS

f4, f8, u2, u8 = np.float32, np.float64, np.uint16, np.uint64
AZ4, AZ2 = np.arange(4.0), np.arange(2.0)


def attach(product, az, n_gates, n_members=None, doppler=True, spectrum=True, staged=('U', 'V', 'W', 'T'), take=None):
    structs, keep = product.attach(N, az, n_gates, n_members, doppler, spectrum, list(staged), take)
    for slot in structs:
        assert slot in dict(N.Outputs._fields_)          # the slot of cpol_outputs its struct hangs on
    return structs


def bind_all(product):
    """Distinct fake addresses into every host array's slot -> {path: address}."""
    bound = {}
    for i, (path, _, _) in enumerate(product.arrays()):
        bound[path] = 0x1000 * (i + 1)
        product.bind(path, bound[path])
    return bound


def pointers(struct, name):
    v = getattr(struct, name)
    return [x or 0 for x in v] if isinstance(v, C.Array) else (v or 0)


# ------------------------------------------------------------------ superobservations
@pytest.mark.parametrize('n_members', [None, 2])
def test_superob_arrays_binding_finish_join(n_members):
    spec = SO.Superob(2, 2)
    p = SO.Windows(spec, keep_gates=False, rays_per_block=2)
    assert (p.name, p.gates, p.spectrum, p.model_var) == ('superob', False, True, None)
    assert SO.Windows(spec, keep_gates=True).gates
    so = attach(p, AZ4, 5, n_members, doppler=False)['superob']
    assert (so.ray_window, so.gate_window, so.rays_per_block, so.min_valid_fraction) == (2, 2, 2, 0.5)
    w = (2, 3) if n_members is None else (2, 2, 3)       # two blocks of one window row; gates 0-1, 2-3 and the short window 4
    nine = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V']
    assert p.arrays() == [(k, f4, w) for k in nine] + [('count', u2, (10,) + w)]
    bound = bind_all(p)
    assert [pointers(so, k) for k in nine + ['count']] == [bound[k] for k in nine + ['count']] and pointers(so, 'RVEL') == 0
    attach(p, AZ4, 5, n_members, doppler=True)
    assert p.arrays()[9] == ('RVEL', f8, w) and len(p.arrays()) == 11
    # device outputs: {field or 'count': pointer}, as they come
    so = attach(p, AZ4, 5, n_members)['superob']
    p.bind_device({'KDP': 7, 'count': 9})
    assert (so.KDP, so.count, so.ZH) == (7, 9, None)
    # the finish: a count row goes to its field, the window coordinates come from the caller's rule, once
    attach(p, AZ4, 5, n_members, doppler=False)
    cnt = np.arange(10)[(slice(None),) + (None,) * len(w)] * np.ones(w, u2)
    asked = []

    def coords(key, make):
        asked.append(key)
        return make({k: np.arange(20.0).reshape(4, 5).astype(f8 if k in ('lats', 'lons') else f4) for k in SO.COORDINATES})
    out = p.finish({'ZH': np.zeros(w, f4), 'count': cnt}, coords)
    assert asked == [(2, 2, 2)] and sorted(out) == ['ZH', 'count', 'dist', 'heights', 'lats', 'lons']
    assert list(out['count']) == nine and all((out['count'][k] == i).all() for i, k in enumerate(nine))
    assert out['lats'].shape == (2, 3) and out['lats'][0, 2] == np.mean([4.0, 9.0])
    # the join: member blocks on the leading axis, the coordinates once
    a, b = dict(out, ZH=np.zeros((1, 2, 3), f4)), dict(out, ZH=np.ones((1, 2, 3), f4))
    a['count'] = b['count'] = {'ZH': np.zeros((1, 2, 3), u2)}
    j = p.join([a, b], np.concatenate)
    assert j['ZH'].shape == (2, 2, 3) and (j['ZH'][1] == 1).all() and j['count']['ZH'].shape == (2, 2, 3)
    assert j['lats'] is a['lats']
    assert p.join([a, b], np.stack)['ZH'].shape == (2, 1, 2, 3)


def test_superob_refusals():
    with pytest.raises(ValueError, match='superob: a cosmo_pol_amd.superob.Superob'):
        SO.Windows((2, 2))
    with pytest.raises(NotImplementedError, match='process group'):
        SO.Windows(SO.Superob(2, 2), distributed=True)
    with pytest.raises(ValueError, match='does not divide the 4 rays'):
        attach(SO.Windows(SO.Superob(2, 2), rays_per_block=3), AZ4, 5)
    with pytest.raises(ValueError, match='does not divide'):
        attach(SO.Windows(SO.Superob(2, 2), rays_per_block=-1), AZ4, 5)
    assert set(SO.Windows.refuses) == {'groups'} and not SO.Windows.over_members


# ------------------------------------------------------------------ ensemble statistics, quantiles, verification
def test_stats_arrays_binding_finish_join():
    spec = EV.EnsembleVerification(verify=['KDP'], quantiles={'ZH': [0.5, 0.9]}, fields=['KDP', 'ZH'], extremes=True,
                                   exceed={'ZH': [1.0, 2.0]})
    obs = {'KDP': np.arange(6, dtype=f4).reshape(2, 3)}
    p = ES.Fold(spec, keep_members=False, phase=3, capacity=5, observations=obs)
    assert (p.name, p.gates, p.spectrum, p.model_var, p.over_members) == ('stats', False, True, None, True)
    taken = []

    def take(block):
        views = [np.zeros(sh, dt) for _, dt, sh in block]
        taken.append((block, views))
        return views, [0x77000 + 64 * i for i in range(len(block))]
    structs = attach(p, AZ2, 3, n_members=2, take=take)
    ms, mv = structs['member_stats'], structs['member_verify']
    zh, kdp = ES.FIELDS.index('ZH'), ES.FIELDS.index('KDP')
    assert ms.fields == (1 << zh) | (1 << kdp) and ms.phase == 3 and ms.quantile_capacity == 5 and mv.fields == 1 << kdp
    # the observations: a clean block of their own, written before the call, bound to the verified field's slot
    assert taken[0][0] == [('KDP', f4, (2, 3))] and (taken[0][1][0] == obs['KDP']).all()
    assert pointers(mv, 'obs') == [0x77000 if i == kdp else 0 for i in range(10)]
    g = (2, 3)
    assert p.arrays() == [
        (('mean', 'ZH'), f4, g), (('mean', 'KDP'), f4, g), (('spread', 'ZH'), f4, g), (('spread', 'KDP'), f4, g),
        (('min', 'ZH'), f4, g), (('min', 'KDP'), f4, g), (('max', 'ZH'), f4, g), (('max', 'KDP'), f4, g),
        ('count', u2, (10, 2, 3)), (('exceed', 'ZH'), u2, (2, 2, 3)), (('quantile', 'ZH'), f4, (2, 2, 3)),
        (('below', 'KDP'), u2, g), (('equal', 'KDP'), u2, g), (('crps', 'KDP'), f4, g)]
    bound = bind_all(p)
    for kind in ('mean', 'spread', 'min', 'max', 'exceed', 'quantile'):
        want = [bound.get((kind, k), 0) for k in ES.FIELDS]
        assert pointers(ms, kind) == want and (want[zh] != 0) and (want[kdp] != 0) == (kind in ES.KINDS)
    for kind in EV.OUTPUTS:
        assert pointers(mv, kind) == [bound[(kind, 'KDP')] if i == kdp else 0 for i in range(10)]
    assert ms.count == bound['count']
    # RVEL: float64, and only with Doppler
    q = ES.Fold(ES.EnsembleStats(spread=False, fields=['RVEL']), capacity=2)
    attach(q, AZ2, 3)
    assert q.arrays() == [(('mean', 'RVEL'), f8, g), ('count', u2, (10, 2, 3))]
    with pytest.raises(ValueError, match='RVEL'):
        attach(q, AZ2, 3, doppler=False)
    # a call that does not finish the pass brings nothing and binds nothing
    p.phase = 1
    ms = attach(p, AZ2, 3, take=take)['member_stats']
    assert p.arrays() == [] and len(taken) == 1
    p.bind_device({'mean': {'ZH': 5}})
    assert pointers(ms, 'mean') == [0] * 10
    # the finish: kinds nested, the verification under 'verify', a count row per folded field, n_members of the pass
    p.phase = 3
    attach(p, AZ2, 3, take=take)
    views = {path: np.zeros(sh, dt) for path, dt, sh in p.arrays()}
    views['count'] = np.arange(10, dtype=u2)[:, None, None] * np.ones(g, u2)
    out = p.finish(views, None)
    assert sorted(out) == ['count', 'exceed', 'max', 'mean', 'min', 'n_members', 'quantile', 'spread', 'verify']
    assert sorted(out['verify']) == ['below', 'crps', 'equal'] and list(out['verify']['crps']) == ['KDP']
    assert sorted(out['count']) == ['KDP', 'ZH'] and (out['count']['KDP'] == kdp).all() and (out['count']['ZH'] == zh).all()
    assert out['n_members'] == 5 and list(out['exceed']) == ['ZH'] and out['mean']['KDP'] is views[('mean', 'KDP')]
    plain = ES.Fold(ES.EnsembleStats(), capacity=None)
    attach(plain, AZ2, 3, doppler=False)
    out = plain.finish({('mean', 'ZH'): 1, 'count': np.zeros((10, 2, 3), u2)}, None)
    assert out['exceed'] == {} and 'quantile' not in out and 'n_members' not in out and len(out['count']) == 9
    # the join: one pass, the finishing call holds it
    assert p.join([None, 'last'], np.concatenate) == 'last'


def test_stats_device_outputs_and_refusals():
    p = ES.Fold(ES.EnsembleStats(fields=['ZH', 'KDP']), capacity=3)
    ms = attach(p, AZ2, 3)['member_stats']
    p.bind_device({'mean': {'KDP': 11}, 'spread': {'ZH': 12}, 'exceed': {'ZH': 13}, 'quantile': {'ZH': 14}, 'count': 15})
    kdp = ES.FIELDS.index('KDP')
    assert pointers(ms, 'mean') == [11 if i == kdp else 0 for i in range(10)]
    assert (ms.spread[0], ms.exceed[0], ms.quantile[0], ms.count) == (12, 13, 14, 15)
    with pytest.raises(ValueError, match="unknown entry 'median'"):
        p.bind_device({'median': {'ZH': 1}})
    for kind in ('obs', 'below', 'equal', 'crps'):
        with pytest.raises(ValueError, match='without an EnsembleVerification'):
            p.bind_device({kind: {'ZH': 1}})
    v = ES.Fold(EV.EnsembleVerification(verify=['ZH']), capacity=3)
    mv = attach(v, AZ2, 3)['member_verify']            # (device outputs: no `take`, the observations are the caller's pointers)
    v.bind_device({'obs': {'ZH': 21}, 'below': {'ZH': 22}, 'equal': {'ZH': 23}, 'crps': {'ZH': 24}})
    assert (mv.obs[0], mv.below[0], mv.equal[0], mv.crps[0]) == (21, 22, 23, 24)
    # the limits of a pass
    with pytest.raises(ValueError, match='ensemble quantiles: at most 128'):
        ES.Fold(ES.EnsembleQuantiles({'ZH': [0.5]}), capacity=129)
    with pytest.raises(ValueError, match='ensemble verification: at most 128'):
        ES.Fold(EV.EnsembleVerification(verify=['ZH']), capacity=129)
    with pytest.raises(ValueError, match='ensemble statistics: at most 65535'):
        ES.Fold(ES.EnsembleStats(), capacity=65536)
    ES.Fold(ES.EnsembleStats(), capacity=65535)
    assert set(ES.Fold.refuses) == {'timed', 'subbeams'} and 'time-blended or sub-beam' in ES.Fold.refuses['timed']


# ------------------------------------------------------------------ spectrum moments
def test_moments_arrays_binding_finish_refusals():
    spec = SM.SpectrumMoments(fields=('VHIGH', 'VMEAN'))          # (not a prefix of the eight, and not in their order)
    p = SM.Rows(spec, keep_spectrum=False, scheme=3)
    assert (p.name, p.gates, p.spectrum, p.model_var) == ('moments', True, False, None) and SM.Rows(spec, True).spectrum
    sm = attach(p, AZ2, 3)['spectrum_moments']
    assert sm.fields == (1 << 1) | (1 << 7)
    assert p.arrays() == [('moments', f8, (8, 2, 3)), ('count', u2, (2, 3))]
    bound = bind_all(p)
    assert (sm.moments, sm.count) == (bound['moments'], bound['count'])
    p.bind_device({'count': 5, 'moments': 6})
    assert (sm.moments, sm.count) == (6, 5)
    with pytest.raises(ValueError, match="unknown entry 'VMEAN'"):
        p.bind_device({'VMEAN': 1})
    rows = np.arange(8.0)[:, None, None] * np.ones((2, 3))
    out = p.finish({'moments': rows, 'count': np.zeros((2, 3), u2)}, None)
    assert sorted(out) == ['VHIGH', 'VMEAN', 'count'] and (out['VMEAN'] == 1).all() and (out['VHIGH'] == 7).all()
    with pytest.raises(ValueError, match='moments: a cosmo_pol_amd.spectrum_moments.SpectrumMoments'):
        SM.Rows(('POWER',))
    with pytest.raises(ValueError, match='doppler scheme 3, configured is 1'):
        SM.Rows(spec, scheme=1)
    with pytest.raises(NotImplementedError, match='process group'):
        SM.Rows(spec, distributed=True)
    with pytest.raises(ValueError, match='this radar simulates none'):
        attach(p, AZ2, 3, spectrum=False)
    assert set(SM.Rows.refuses) == {'members', 'timed', 'subbeams'} and not hasattr(SM.Rows, 'join')


# ------------------------------------------------------------------ histograms
@pytest.mark.parametrize('rpb, nb', [(0, 1), (2, 2)])
def test_histogram_arrays_binding_finish_join(rpb, nb):
    one = HG.Histogram({'RVEL': [0.0, 1.0, 2.0], 'ZV': [0.0, 1.0]})                                  # given against the order of FIELDS
    two = HG.Histogram({'KDP': [0.0, 1.0, 2.0, 3.0]}, ordinate=('model', 'T'), ordinate_edges=[0.0, 1.0, 2.0])
    p = HG.Counts(one, keep_gates=False, phase=3, rays_per_block=rpb)
    assert (p.name, p.gates, p.spectrum, p.model_var) == ('histogram', False, True, None)
    h = attach(p, AZ4, 5)['histogram']
    assert (h.fields, h.phase, h.rays_per_block) == ((1 << 1) | (1 << 9), 3, rpb)
    assert p.arrays() == [('ZV', u8, (nb, 3)), ('RVEL', u8, (nb, 4))]
    bound = bind_all(p)
    assert pointers(h, 'counts') == [bound.get(k, 0) for k in HG.FIELDS]
    q = HG.Counts(two, keep_gates=True, phase=2, rays_per_block=rpb)
    assert q.gates and q.model_var == 'T'
    h = attach(q, AZ4, 5, n_members=None)['histogram']
    assert h.ordinate == HG.ORD_MODEL + 3 and q.arrays() == [('KDP', u8, (nb, 4, 5))]
    q.bind_device({'KDP': 9})
    assert pointers(h, 'counts') == [9 if k == 'KDP' else 0 for k in HG.FIELDS]
    # an ensemble call: the rows of all members
    attach(p, AZ4, 5, n_members=3)
    assert p.arrays()[0] == ('ZV', u8, (3 * nb if rpb else 1, 3))
    # a call that does not finish the pass
    p.phase = 1
    h = attach(p, AZ4, 5)['histogram']
    p.bind_device({'ZV': 5})
    assert p.arrays() == [] and pointers(h, 'counts') == [0] * 10
    # the finish and the join
    out = q.finish({'KDP': np.ones((nb, 4, 5), u8)}, None)
    assert sorted(out) == ['counts', 'edges', 'ordinate_edges'] and out['edges']['KDP'] is two.edges['KDP']
    assert out['ordinate_edges'] is two.ordinate_edges and list(out['counts']) == ['KDP']
    j = q.join([out, dict(out, counts={'KDP': np.zeros((nb, 4, 5), u8)})], np.concatenate)
    if rpb:                               # a block per member: joined on the leading axis
        assert j['counts']['KDP'].shape == (2 * nb, 4, 5) and j['counts']['KDP'][:nb].all() and not j['counts']['KDP'][nb:].any()
    else:                                 # one pass: the last call's
        assert not j['counts']['KDP'].any()
    assert j['edges'] is out['edges']


def test_histogram_refusals():
    with pytest.raises(ValueError, match='hist: a cosmo_pol_amd.histogram.Histogram'):
        HG.Counts({'ZH': [0, 1]})
    spec = HG.Histogram({'ZH': [0.0, 1.0]}, ordinate='RVEL', ordinate_edges=[0.0, 1.0])
    with pytest.raises(ValueError, match='RVEL needs a Doppler scheme'):
        HG.Counts(spec, doppler=False)
    with pytest.raises(ValueError, match='RVEL needs a Doppler scheme'):
        HG.Counts(HG.Histogram({'RVEL': [0.0, 1.0]}), doppler=False)
    HG.Counts(HG.Histogram({'ZH': [0.0, 1.0]}), doppler=False)
    with pytest.raises(NotImplementedError, match='process group'):
        HG.Counts(spec, distributed=True)
    with pytest.raises(ValueError, match='does not divide the 4 rows'):
        attach(HG.Counts(spec, rays_per_block=3), AZ4, 5)
    assert set(HG.Counts.refuses) == {'subbeams', 'groups'} and CP.Maps.refuses is HG.Counts.refuses


# ------------------------------------------------------------------ composites
def test_composite_arrays_binding_finish_join():
    spec = CP.Composite(['KDP', 'ZH'], [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0], products=('max', 'echo_top'),
                        thresholds={'ZH': [1.0], 'KDP': [1.0, 2.0]})                               # a 2 x 3 grid
    p = CP.Maps(spec, keep_gates=False, phase=3, rays_per_block=2)
    assert (p.name, p.gates, p.spectrum, p.model_var) == ('composite', False, True, None)
    c = attach(p, AZ4, 5)['composite']
    assert (c.fields, c.phase, c.rays_per_block, c.n_x, c.n_y) == (0b1001, 3, 2, 3, 2) and c.ray_sin and c.ray_cos
    assert p.arrays() == [('ZH', f4, (2, 3, 2, 3)), ('KDP', f4, (2, 4, 2, 3)), ('count', u8, (2, 2, 2, 3))]
    bound = bind_all(p)
    assert pointers(c, 'values') == [bound.get(k, 0) for k in CP.FIELDS] and c.count == bound['count']
    p.bind_device({'values': {'KDP': 5}, 'count': 6})
    assert pointers(c, 'values') == [bound['ZH'], 0, 0, 5, 0, 0, 0, 0, 0] and c.count == 6
    with pytest.raises(ValueError, match="unknown entry 'ZH'"):
        p.bind_device({'ZH': 1})
    p.phase = 0
    c = attach(p, AZ4, 5)['composite']
    p.bind_device({'count': 6, 'nonsense': 1})          # (a call that does not finish the pass reads no entry)
    assert p.arrays() == [] and not c.count
    with pytest.raises(ValueError, match='spec: a cosmo_pol_amd.composite.Composite'):
        CP.Maps(['ZH'])
    with pytest.raises(NotImplementedError, match='process group'):
        CP.Maps(spec, distributed=True)
    with pytest.raises(ValueError, match='does not divide the 8 rows'):
        attach(CP.Maps(spec, rays_per_block=3), AZ4, 5, n_members=2)
    # the finish: the planes split by name, a count plane per field; the join: blocks on the leading axis
    views = {'ZH': np.arange(3, dtype=f4)[None, :, None, None] * np.ones((2, 3, 2, 3), f4),
             'KDP': np.arange(4, dtype=f4)[None, :, None, None] * np.ones((2, 4, 2, 3), f4),
             'count': np.arange(2, dtype=u8)[None, :, None, None] * np.ones((2, 2, 2, 3), u8)}
    out = p.finish(views, None)
    assert sorted(out) == ['count', 'values', 'x_edges', 'y_edges'] and out['x_edges'] is spec.x_edges
    assert list(out['values']['ZH']) == ['max', 'height_of_max', 'echo_top_0']
    assert list(out['values']['KDP']) == ['max', 'height_of_max', 'echo_top_0', 'echo_top_1']
    assert (out['values']['KDP']['echo_top_1'] == 3).all() and out['values']['ZH']['max'].shape == (2, 2, 3)
    assert (out['count']['ZH'] == 0).all() and (out['count']['KDP'] == 1).all()
    p.rays_per_block = 2
    j = p.join([out, out], np.concatenate)
    assert j['values']['ZH']['max'].shape == (4, 2, 3) and j['count']['KDP'].shape == (4, 2, 3) and j['y_edges'] is spec.y_edges
    p.rays_per_block = 0
    assert p.join([None, out], np.concatenate)['values'] is out['values']


# ------------------------------------------------------------------ the operator's side
def test_device_output_entries_name_every_product():
    names = {cls.name for cls in (SO.Windows, ES.Fold, SM.Rows, HG.Counts, CP.Maps)}
    assert set(_PRODUCT_OUTPUTS) == names == {'superob', 'stats', 'moments', 'histogram', 'composite'}
    assert not names & set(N.OUTPUT_FIELDS) - {'histogram', 'composite'}


def test_block_packer():
    class Pool(object):
        def take(self, nbytes, writer=None):
            self.asked = (nbytes, writer)
            return np.zeros(nbytes + 64, np.uint8), {'ctx': None, 'serial': 0}
    pool = Pool()
    spec = [('a', np.float32, (3, 5)), ('b', np.float64, (2, 1, 3)), ('c', np.int8, (7,)), ('d', np.uint16, (3, 3)),
            ('e', np.uint64, (1,)), ('f', np.float32, (0, 4))]
    views, addresses, holder = N.carve_block(pool, spec, writer='lane')
    assert pool.asked == (64 + 64 + 64 + 64 + 64 + 0, 'lane') and holder == {'ctx': None, 'serial': 0}
    base = addresses[0]
    assert [a - base for a in addresses] == [0, 64, 128, 192, 256, 320]
    for (_, dt, sh), v, a in zip(spec, views, addresses):
        assert v.dtype == dt and v.shape == sh and (v.size == 0 or v.ctypes.data == a)
    ends = [a + v.nbytes for v, a in zip(views, addresses)]
    assert all(e <= nxt for e, nxt in zip(ends, addresses[1:]))          # no overlap
    for i, v in enumerate(views):
        v[...] = i + 1
    assert all((v == i + 1).all() for i, v in enumerate(views))
