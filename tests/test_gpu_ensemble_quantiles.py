"""Ensemble quantiles on the GPU (cpol_member_stats.quantile_*, the stash of k_member_fold and k_member_quantile) against
ensemble_stats (the NumPy statement of the rule), bit for bit -- the rule is exact, so there is no tolerance; NaNs compare equal
whatever their payload.  First the kernels on explicit members through the test hook (cpol_debug_read "member_stats_fields":
sizes at the edges of the one-wavefront workgroup, passes cut into calls up to the cap of 128 members, every value class, every
method), the invariances and the refusals; then end to end: simulate_rays_ensemble_stats with an EnsembleQuantiles against
ensemble_stats.reduce(simulate_rays_ensemble(...)) on the three members of tests/test_gpu_ensemble.py."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_ensemble as E
import test_gpu_ensemble_stats as S

pytestmark = pytest.mark.gpu

FIELDS = S.FIELDS
N_CELLS = [1, 63, 64, 65, 127, 128, 129, 1031]
PASSES = [[1], [2], [3], [21], [64, 1], [64, 64], [1, 1, 1, 1, 1]]
CLASSES = S.CLASSES + ['ties']
POOL = [0.0, 1.0, 0.5, 0.1, 0.9, 1.0 / 3.0, 0.25, 0.75]     # (h = q (n - 1) is a whole number for some n: 0.5 at odd n, 0.25 at n = 5, ...)
SETS = [(['ZH'], ['ZH']), (['RVEL'], ['RVEL']), (FIELDS, ['ZH', 'KDP', 'RVEL'])]        # (folded fields, those with quantiles)


@pytest.fixture(scope='module', autouse=True)
def _close_operators(request):
    """The operators are those of tests/test_gpu_ensemble_stats.py (S.ens_op); that module closes them after its own tests,
    this one when it runs without it."""
    yield
    if not any(getattr(item, 'module', None) is S for item in request.session.items):
        for op in S._ops.values():
            op.close()
        S._ops.clear()


def members_of(cls, M, n_cells, T, need, rng):
    if cls != 'ties':
        return S.members_of(cls, M, n_cells, T, need, rng)
    x = S.members_of('random', M, n_cells, T, need, rng)
    ties = rng.choice(np.array([1.5, -2.0, 0.25, 1e3]), x.shape).astype(T)
    keep = np.isnan(x) | (np.arange(n_cells) < 3)[None]     # (the NaNs and the cells with a planted count stay)
    return np.where(keep, x, ties)


def run_pass(ctx, rows, spec, cut, capacity=None):
    at, got = 0, None
    for j, n in enumerate(cut):
        phase = (1 if j == 0 else 0) | (2 if j == len(cut) - 1 else 0)
        got = ctx.member_stats_fields({k: v[at:at + n] for k, v in rows.items()}, spec, phase=phase,
                                      capacity=sum(cut) if capacity is None else capacity)
        assert (got is None) == (j < len(cut) - 1)
        at += n
    return got


@pytest.mark.parametrize('n_cells', N_CELLS)
def test_hook_against_the_rule(n_cells):
    from cosmo_pol_amd import ensemble_stats as ES
    ctx = S.ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(2000 + n_cells)
    seen, i = set(), 0
    for cut in PASSES:
        for cls in CLASSES:
            t = i % 24
            (names, with_q), n_q, method = SETS[t % 3], (1, 8)[(t // 3) % 2], ES.METHODS[t // 6]
            need = (1, 2, 3)[(i + i // 24) % 3]
            M = sum(cut)
            rows = {k: members_of(cls, M, n_cells, ES.dtype_of(k), need, rng) for k in names}
            q = {k: (POOL if n_q == 8 else [POOL[(i + j) % 8]]) for j, k in enumerate(with_q)}
            spec = ES.EnsembleQuantiles(q, method=method, extremes=True, fields=names, min_members=need,
                                        exceed={names[0]: [0.0, 1.0]})
            with np.errstate(all='ignore'):
                want = ES.reduce(rows, spec)
            tag = '%d cells, %r, %s, %d field(s), %d q, %s, need %d' % (n_cells, cut, cls, len(names), n_q, method, need)
            got = run_pass(ctx, rows, spec, cut)
            # every array: the quantiles, and the other statistics of the same pass
            assert S.assert_stats(got, want, tag) == len(names) * 5 + 1 + len(with_q), tag
            assert set(got) == set(want) - {'n_members'} and got['quantile'][with_q[0]].shape == (n_q, n_cells), tag
            seen.add((t % 3, n_q, method))
            if n_cells > 2 and M >= need:
                w = want['quantile'][with_q[0]]
                assert np.isnan(w[:, :2]).all() and (w[:, 2] == 1.5).all(), tag
            i += 1
    assert len(seen) == 24 and i == 42


def test_hook_invariances_and_no_leak_into_the_next_pass():
    from cosmo_pol_amd import ensemble_stats as ES
    ctx = S.ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(17)
    M, n_cells = 21, 300
    for cls, method in (('random', 'linear'), ('negzero', 'lower'), ('ties', 'nearest'), ('inf', 'linear'), ('decades', 'higher')):
        rows = {k: members_of(cls, M, n_cells, ES.dtype_of(k), 2, rng) for k in ('ZH', 'RVEL')}
        spec = ES.EnsembleQuantiles({'ZH': POOL, 'RVEL': [0.5, 0.9]}, method=method, fields=['ZH', 'RVEL'], min_members=2)
        with np.errstate(all='ignore'):
            want = ES.reduce(rows, spec)
        first = run_pass(ctx, rows, spec, [M])
        S.assert_stats(first, want, cls)
        # the members permuted: the same quantile bits (the mean's last bits may differ: not compared)
        p = rng.permutation(M)
        got = run_pass(ctx, {k: v[p] for k, v in rows.items()}, spec, [M])
        for k in rows:
            assert S.same(got['quantile'][k], first['quantile'][k]), (cls, 'permuted', k)
            assert S.same(got['count'][k], first['count'][k])
        # the pass cut differently: the same bits of everything; a capacity above the members folded changes nothing
        for cut, cap in (([1] * M, None), ([20, 1], None), ([1, 20], 128), ([7, 0, 14], 22)):
            S.assert_stats(run_pass(ctx, rows, spec, cut, capacity=cap), want, (cls, cut, cap))
        # a pass without quantiles straight after one with: what tests/test_gpu_ensemble_stats.py expects of it
        plain = ES.EnsembleStats(extremes=True, exceed={'ZH': [0.0, 1.0]}, fields=['ZH', 'RVEL'], min_members=2)
        with np.errstate(all='ignore'):
            want_plain = ES.reduce(rows, plain)
        got = ctx.member_stats_fields(rows, plain)
        assert 'quantile' not in got and S.assert_stats(got, want_plain, cls + ', plain afterwards') == 2 * 5 + 1
        got = ctx.member_stats_fields({k: v[:10] for k, v in rows.items()}, plain, phase=1)
        got = ctx.member_stats_fields({k: v[10:] for k, v in rows.items()}, plain, phase=2)
        S.assert_stats(got, want_plain, cls + ', plain afterwards, cut')
    # a pass with quantiles that folds no member at all, and one finished without members
    spec = ES.EnsembleQuantiles({'ZH': [0.5]}, fields=['ZH'])
    empty = ctx.member_stats_fields({}, spec, phase=3, n_cells=n_cells, names=('ZH',))
    assert np.isnan(empty['quantile']['ZH']).all() and empty['quantile']['ZH'].shape == (1, n_cells)
    zh = {'ZH': rows['ZH']}
    assert ctx.member_stats_fields(zh, spec, phase=1) is None
    got = ctx.member_stats_fields({}, spec, phase=2, n_cells=n_cells, names=('ZH',), capacity=M)
    with np.errstate(all='ignore'):
        S.assert_stats(got, ES.reduce(zh, spec), 'finish without members')


def q_hook(ctx, x, phase, change=None, capacity=5, method=0, q=(0.25, 0.5), outputs=True, q_output=True):
    """S.raw_hook (ZH alone, two thresholds) with quantile terms; `change(h, keep)` spoils them.  -> (rc, outputs)"""
    qa = np.array(q, dtype=np.float64)
    qout = np.full((len(q), np.shape(x)[1]), 77, np.float32)

    def fill(h, keep):
        keep.append(qa)
        h.ms.quantile_capacity, h.ms.quantile_method = capacity, method
        h.ms.n_quantiles[0], h.ms.quantiles[0] = len(qa), qa.ctypes.data
        if q_output:
            h.ms.quantile[0] = qout.ctypes.data
        if change is not None:
            change(h, keep)
    rc, out = S.raw_hook(ctx, x, fill, phase, outputs=outputs)
    out['quantile'] = qout
    return rc, out


def test_hook_refusals_leave_the_open_pass_alone():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import ensemble_stats as ES
    ctx = S.ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(5)
    x = S.members_of('random', 5, 129, np.float32, 1, rng)
    spec = ES.EnsembleQuantiles({'ZH': [0.25, 0.5]}, extremes=True, exceed={'ZH': [1.0, 1.5]}, fields=['ZH'])
    want = ES.reduce({'ZH': x}, spec)
    few = x[3:]

    def s(**kw):
        def change(h, keep):
            for k, v in kw.items():
                if k == 'n_q':
                    h.ms.n_quantiles[0] = v
                elif k == 'n_q_other':
                    h.ms.n_quantiles[4] = v                 # (a field that is not folded: the range is checked all the same)
                elif k == 'q':
                    keep.append(v)
                    h.ms.quantiles[0] = None if v is None else v.ctypes.data
                else:
                    setattr(h.ms, k, v)
        return change
    arr = lambda *v: np.array(v, dtype=np.float64)
    # (what is wrong, the phase of the refused call, its members)
    bad = [(s(quantile_method=4), 0, few), (s(quantile_method=-1), 1, few), (s(quantile_method=4), 3, few),
           (s(quantile_capacity=129), 0, few), (s(quantile_capacity=-1), 1, few), (s(quantile_capacity=0), 1, few),
           (s(quantile_capacity=0), 0, few), (s(n_q=9), 1, few), (s(n_q=-1), 0, few), (s(n_q_other=9), 1, few), (s(q=None), 1, few),
           (s(q=arr(0.25, np.nan)), 1, few), (s(q=arr(0.25, 1.5)), 0, few), (s(q=arr(-0.1, 0.5)), 3, few),
           # a fold that differs from the open pass: capacity, method, the number of quantiles, their values
           (s(quantile_capacity=6), 0, few), (s(quantile_method=1), 2, few), (s(n_q=1), 0, few), (s(q=arr(0.25, 0.75)), 2, few),
           # beyond the capacity: in the middle of a pass (3 of 5 are folded), in a finishing call, in a call that begins a pass
           (None, 0, x[:3]), (None, 2, x[:3]), (None, 1, np.zeros((6, 129), np.float32)), (None, 3, np.zeros((6, 129), np.float32))]
    for i, (change, phase, rows) in enumerate(bad):
        assert q_hook(ctx, x[:3], 1)[0] == 0
        rc, out = q_hook(ctx, rows, phase, change)
        assert rc == N.ERR_ARG, (i, phase, rc)
        assert (out['mean'] == 77).all() and (out['count'] == 77).all() and (out['quantile'] == 77).all(), i
        rc, out = q_hook(ctx, few, 2)
        assert rc == 0
        got = {k: {'ZH': out[k]} for k in ('mean', 'spread', 'min', 'max', 'exceed', 'quantile')}
        got['count'] = {'ZH': out['count'][0]}
        S.assert_stats(got, want, 'after refusal %d' % i)
    # a finishing call whose only output pointers are quantile pointers is a finishing call; with none at all it is refused
    assert q_hook(ctx, x[:3], 1)[0] == 0
    assert q_hook(ctx, few, 2, outputs=False, q_output=False)[0] == N.ERR_ARG
    rc, out = q_hook(ctx, few, 2, outputs=False)
    assert rc == 0 and S.same(out['quantile'], want['quantile']['ZH']) and (out['mean'] == 77).all()
    # an unwanted quantile output (NULL) beside the others
    rc, out = q_hook(ctx, x, 3, q_output=False)
    assert rc == 0 and S.same(out['mean'], want['mean']['ZH']) and (out['quantile'] == 77).all()
    # a capacity without quantiles is no pass with quantiles: more members than it are folded
    rc, out = q_hook(ctx, x, 3, s(n_q=0), capacity=2)
    assert rc == 0 and S.same(out['mean'], want['mean']['ZH']) and (out['quantile'] == 77).all()
    with pytest.raises(ValueError, match='quantile_capacity'):
        ctx.member_stats_fields({'ZH': x}, spec, capacity=4)
    S.assert_stats(ctx.member_stats_fields({'ZH': x}, spec), want, 'at the end')


# ---------------------------------------------------------------- end to end
def q_spec(method='linear', **kw):
    from cosmo_pol_amd import ensemble_stats as ES
    return ES.EnsembleQuantiles({'ZH': [0.1, 0.5, 0.9], 'RVEL': 0.5}, method=method, extremes=True,
                                exceed={'ZH': [ES.dbz(0.0), ES.dbz(20.0)]}, min_members=2, **kw)


@pytest.mark.parametrize('name', S.NAMES)
def test_end_to_end(name):
    import torch
    from cosmo_pol_amd import ensemble_stats as ES
    op = S.ens_op(name)
    _, _, _, az, el = E.case(name)
    full = op.simulate_rays_ensemble(az, el, form='shared')
    full = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in full.items()}
    if 'RVEL' in full:
        spec = q_spec()
    else:                                                   # (no Doppler scheme in this case: the median of KDP instead)
        spec = ES.EnsembleQuantiles({'ZH': [0.1, 0.5, 0.9], 'KDP': 0.5}, extremes=True,
                                    exceed={'ZH': [ES.dbz(0.0), ES.dbz(20.0)]}, min_members=2)
    assert name != 'c2_rsg' or 'RVEL' in full
    with np.errstate(all='ignore'):
        want = ES.reduce(full, spec)
    shape = full['ZH'].shape[1:]
    assert want['quantile']['ZH'].shape == (3,) + shape and set(want['quantile']) == set(spec.quantiles)
    c = want['count']['ZH']
    assert ((c > 0) & (c < 3)).any() and (c == 3).any() and np.isfinite(want['quantile']['ZH']).any()
    for form in ('shared', 'per_member'):
        tag = '%s/%s' % (name, form)
        # blocking
        got = op.simulate_rays_ensemble_stats(az, el, spec, form=form)
        assert 'ZH' not in got and got['stats']['n_members'] == 3 and set(got['stats']) == set(want)
        S.assert_stats(got['stats'], want, tag)
        for k in S.GEOM:
            assert S.same(got[k], full[k]), (form, k)
        # page-locked buffers on another lane: the one-copy window
        got = op.simulate_rays_ensemble_stats(az, el, spec, form=form, lane=1, pinned=True)
        op.wait(1)
        S.assert_stats(got['stats'], want, tag + '/pinned on lane 1')
        # device outputs for the quantiles (the other statistics stay NULL: quantile pointers alone finish the pass)
        dev = {k: torch.full(v.shape, 7, dtype=torch.float64 if k == 'RVEL' else torch.float32, device='cuda')
               for k, v in want['quantile'].items()}
        res = op.simulate_rays_ensemble_stats(az, el, spec, form=form, lane=1,
                                              device_outputs={'stats': {'quantile': {k: a.data_ptr() for k, a in dev.items()}}})
        op.wait(1)
        assert 'ZH' not in res
        for k, a in dev.items():
            assert S.same(a.cpu().numpy(), want['quantile'][k]), (tag, 'device outputs', k)
        # keep_members
        kept = op.simulate_rays_ensemble_stats(az, el, spec, keep_members=True, form=form)
        S.assert_stats(kept['stats'], want, tag + '/keep_members')
        for k, v in full.items():
            if isinstance(v, np.ndarray):
                assert S.same(kept[k], v), (form, k)
    # a budget that cuts the members into chunks
    try:
        op.sequence_memory_budget = 1
        got = op.simulate_rays_ensemble_stats(az, el, spec, form='shared')
        S.assert_stats(got['stats'], want, name + '/one member per chunk')
    finally:
        op.sequence_memory_budget = None
    # the member order does not matter to the quantiles; another method
    got = op.simulate_rays_ensemble_stats(az, el, spec, members=[2, 0, 1])['stats']
    for k in want['quantile']:
        assert S.same(got['quantile'][k], want['quantile'][k]), k
    near = ES.EnsembleQuantiles({'ZH': [0.5]}, method='nearest', mean=False, spread=False, fields=['ZH'])
    got = op.simulate_rays_ensemble_stats(az, el, near)['stats']
    assert set(got) == {'count', 'exceed', 'quantile', 'n_members'}
    with np.errstate(all='ignore'):
        S.assert_stats(got, ES.reduce(full, near), name + '/nearest')
        assert S.same(ES.db(got['quantile']['ZH']), ES.quantiles(ES.db(full['ZH']), [0.5], 'nearest'))


def test_the_calls_around_and_the_scan():
    from cosmo_pol_amd import ensemble_stats as ES
    name = 'c2_rsg'
    op = S.ens_op(name)
    _, _, _, az, el = E.case(name)
    spec = q_spec('lower')
    for _ in range(3):                                      # (three times: a single-beam sweep replays its gate stencil from the third)
        one = {k: np.array(v) for k, v in op.simulate_rays(az, el).items() if isinstance(v, np.ndarray)}
    forms_one = op._ctx.launch_forms()
    for form in ('shared', 'per_member'):
        op.simulate_rays_ensemble_stats(az, el, spec, form=form)
        after = op.simulate_rays(az, el)
        assert op._ctx.launch_forms() == forms_one, form
        for k, v in one.items():
            assert S.same(after[k], v), (form, 'simulate_rays afterwards', k)
    # more than 128 members: refused before anything runs (nothing is even validated against the staged members)
    ran = []
    orig = op._run_rays
    op._run_rays = lambda *a, **kw: ran.append(1) or orig(*a, **kw)
    try:
        with pytest.raises(ValueError, match='quantiles: at most 128'):
            op.simulate_rays_ensemble_stats(az, el, spec, members=list(range(129)))
        with pytest.raises(ValueError, match='staged'):     # (a plain spec has no such limit: the member list is checked as ever)
            op.simulate_rays_ensemble_stats(az, el, S.stats_spec(), members=list(range(129)))
    finally:
        del op._run_rays
    assert not ran
    # a PPI over two lanes returns the quantile entry
    op2 = S.ens_op(name, lanes=2)
    azimuths = az[0] + 0.5 * np.arange(3)
    elevations = [el[0], el[0] + 0.7]
    scans = op2.get_PPI_ensemble_stats(elevations, spec, azimuths=azimuths, members=[1, 2, 0])
    assert len(scans) == 2
    for e, res in zip(elevations, scans):
        want = S.reference(op2, azimuths, np.full(3, e), spec, members=[1, 2, 0])[0]
        assert res['stats']['quantile']['ZH'].shape == (3, 3, want['mean']['ZH'].shape[1])
        S.assert_stats(res['stats'], want, 'PPI at %.1f' % e)
