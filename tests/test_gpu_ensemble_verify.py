"""Ensemble verification on the GPU (cpol_outputs.member_verify, k_member_verify) against ensemble_verify (the NumPy statement of
the rule), bit for bit -- the rule is exact, so there is no tolerance; NaNs compare equal whatever their payload.  First the
kernel on explicit members and observations through the test hook (cpol_debug_read "member_verify_fields": sizes at the edges of
the one-wavefront workgroup, passes cut into calls up to the cap of 128 members, every value class of members and observations,
fair or not, with and without quantiles beside it), the invariances and the refusals; then end to end:
simulate_rays_ensemble_verify against ensemble_verify.reduce(simulate_rays_ensemble(...)) on the three members of
tests/test_gpu_ensemble.py."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_ensemble as E
import test_gpu_ensemble_quantiles as Q
import test_gpu_ensemble_stats as S

pytestmark = pytest.mark.gpu

FIELDS = S.FIELDS
N_CELLS = [1, 63, 64, 65, 129, 1031]
PASSES = [[1], [2], [3], [21], [64, 64], [1, 1, 1, 1, 1]]
CLASSES = S.CLASSES + ['ties']
OBS_CLASSES = ['nan', '-inf', '+inf', 'own', '-0', '+0', 'mid', 'below', 'above']
SETS = [(['ZH'], ['ZH']), (['RVEL'], ['RVEL']), (FIELDS, ['ZH', 'KDP', 'RVEL'])]        # (folded fields, verified fields)
OUT = ('below', 'equal', 'crps')


@pytest.fixture(scope='module', autouse=True)
def _close_operators(request):
    """The operators are those of tests/test_gpu_ensemble_stats.py (S.ens_op); that module closes them after its own tests,
    this one when it runs without it."""
    yield
    if not any(getattr(item, 'module', None) in (S, Q) for item in request.session.items):
        for op in S._ops.values():
            op.close()
        S._ops.clear()


def observations_of(x, shift):
    """[n_cells] in x's type: the observation classes cycling over the cells, starting at class `shift`"""
    from cosmo_pol_amd import ensemble_stats as ES
    T = x.dtype.type
    M, n_cells = x.shape
    n = (x == x).sum(axis=0)
    if M:
        xs = np.take_along_axis(x, np.argsort(ES.order_key(x), axis=0, kind='stable'), axis=0)
        at = lambda i: np.take_along_axis(xs, np.clip(i, 0, M - 1)[None], axis=0)[0]
        lo, hi, own = at(np.zeros(n_cells, np.int64)), at(n - 1), at(n // 2)
    else:
        lo = hi = own = np.full(n_cells, np.nan, T)
    with np.errstate(all='ignore'):
        made = {'nan': np.full(n_cells, np.nan, T), '-inf': np.full(n_cells, -np.inf, T), '+inf': np.full(n_cells, np.inf, T),
                'own': np.where(n > 0, own, T(1.5)), '-0': np.full(n_cells, -0.0, T), '+0': np.full(n_cells, 0.0, T),
                'mid': np.where(n > 1, (lo * T(0.5) + hi * T(0.5)).astype(T), T(0.25)),
                'below': np.where(n > 0, (lo - np.abs(lo) - T(1)).astype(T), T(-1)),
                'above': np.where(n > 0, (hi + np.abs(hi) + T(1)).astype(T), T(1))}
    cls = (np.arange(n_cells) + shift) % len(OBS_CLASSES)
    y = np.empty(n_cells, T)
    for j, name in enumerate(OBS_CLASSES):
        y[cls == j] = made[name][cls == j]
    return y


def run_pass(ctx, rows, obs, spec, cut, capacity=None):
    at, got = 0, None
    for j, n in enumerate(cut):
        last = j == len(cut) - 1
        got = ctx.member_verify_fields({k: v[at:at + n] for k, v in rows.items()}, obs if last else None, spec,
                                       phase=(1 if j == 0 else 0) | (2 if last else 0),
                                       capacity=sum(cut) if capacity is None else capacity,
                                       n_cells=next(iter(rows.values())).shape[1], names=tuple(rows))
        assert (got is None) == (not last)
        at += n
    return got


def assert_result(got, want, tag):
    """statistics, quantiles and the three verification outputs: the same entries, dtype, shape, bits"""
    got, want = dict(got), dict(want)
    gv, wv = got.pop('verify'), want.pop('verify')
    n = S.assert_stats(got, want, tag)
    assert set(gv) == set(wv) == set(OUT), tag
    for kind in OUT:
        assert set(gv[kind]) == set(wv[kind]), (tag, kind)
        for k, v in wv[kind].items():
            g = np.asarray(gv[kind][k])
            bad = int((~((g == v) | ((g != g) & (v != v)))).sum()) if g.shape == v.shape else -1
            assert S.same(g, v), (tag, kind, k, g.dtype, v.dtype, g.shape, v.shape, bad)
            n += 1
    return n


@pytest.mark.parametrize('n_cells', N_CELLS)
def test_hook_against_the_rule(n_cells):
    from cosmo_pol_amd import ensemble_stats as ES
    from cosmo_pol_amd import ensemble_verify as EV
    ctx = S.ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(3000 + n_cells)
    seen, i = set(), 0
    for cut in PASSES:
        for cls in CLASSES:
            t = i + 7 * N_CELLS.index(n_cells)              # (every size pairs the classes and cuts with other terms)
            (names, verified), fair, q_mode = SETS[t % 3], bool((t // 3) % 2), (t // 6) % 3
            need = (1, 2, 3)[(i + i // 6) % 3]
            M = sum(cut)
            rows = {k: Q.members_of(cls, M, n_cells, ES.dtype_of(k), need, rng) for k in names}
            obs = {k: observations_of(rows[k], i + j) for j, k in enumerate(verified)}
            # quantiles beside the verification: none; on a verified field (one stash serves both); on another field where there is one
            q = {} if q_mode == 0 else {verified[0]: [0.5, 0.9]} if q_mode == 1 else {names[1] if len(names) > 1 else names[0]: [0.25]}
            spec = EV.EnsembleVerification(verify=verified, fair=fair, quantiles=q, method=ES.METHODS[i % 4], extremes=True, fields=names,
                                           min_members=need, exceed={names[0]: [0.0, 1.0]})
            with np.errstate(all='ignore'):
                want = EV.reduce(rows, obs, spec)
            tag = '%d cells, %r, %s, %d field(s), fair %d, q %d, need %d' % (n_cells, cut, cls, len(names), fair, q_mode, need)
            got = run_pass(ctx, rows, obs, spec, cut)
            # every array: the verification, and the statistics and quantiles of the same pass
            assert assert_result(got, want, tag) == len(names) * 5 + 1 + len(q) + 3 * len(verified), tag
            seen.add((t % 3, fair, q_mode))
            if n_cells > 2 and M >= need:
                w = want['verify']
                k = verified[0]
                assert np.isnan(w['crps'][k][:2]).all(), tag        # (no counting member; need - 1 of them)
                y2 = obs[k][2]
                assert np.isnan(w['crps'][k][2]) == bool(y2 != y2 or (fair and need < 2)), tag
                assert w['below'][k][0] == 0 and w['equal'][k][0] == 0 and w['below'][k][2] + w['equal'][k][2] <= need, tag
            i += 1
    assert len(seen) == 18 and i == 36


def test_hook_invariances_and_no_leak_into_the_next_pass():
    from cosmo_pol_amd import ensemble_stats as ES
    from cosmo_pol_amd import ensemble_verify as EV
    ctx = S.ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(23)
    M, n_cells = 21, 300
    for cls, fair in (('random', False), ('negzero', True), ('ties', False), ('inf', True), ('decades', False)):
        rows = {k: Q.members_of(cls, M, n_cells, ES.dtype_of(k), 2, rng) for k in ('ZH', 'RVEL')}
        obs = {k: observations_of(v, j) for j, (k, v) in enumerate(rows.items())}
        spec = EV.EnsembleVerification(verify=('ZH', 'RVEL'), fair=fair, quantiles={'ZH': [0.5]}, fields=['ZH', 'RVEL'], min_members=2)
        with np.errstate(all='ignore'):
            want = EV.reduce(rows, obs, spec)
        first = run_pass(ctx, rows, obs, spec, [M])
        assert_result(first, want, cls)
        # the members permuted: the same bits of the three outputs (the mean's last bits may differ: not compared)
        p = rng.permutation(M)
        got = run_pass(ctx, {k: v[p] for k, v in rows.items()}, obs, spec, [M])
        for k in rows:
            for kind in OUT:
                assert S.same(got['verify'][kind][k], first['verify'][kind][k]), (cls, 'permuted', kind, k)
        # the pass cut four ways, a call with zero members among them; a capacity above the members folded changes nothing
        for cut, cap in (([1] * M, None), ([20, 1], None), ([1, 20], 128), ([7, 0, 14], 22)):
            assert_result(run_pass(ctx, rows, obs, spec, cut, capacity=cap), want, (cls, cut, cap))
        # a plain pass and a pass with quantiles straight afterwards: what they give without a verification before them
        plain = ES.EnsembleStats(extremes=True, exceed={'ZH': [0.0, 1.0]}, fields=['ZH', 'RVEL'], min_members=2)
        with np.errstate(all='ignore'):
            want_plain = ES.reduce(rows, plain)
        got = ctx.member_stats_fields(rows, plain)
        assert 'quantile' not in got and 'verify' not in got and S.assert_stats(got, want_plain, cls + ', plain afterwards') == 2 * 5 + 1
        quant = ES.EnsembleQuantiles({'RVEL': [0.1, 0.5]}, fields=['ZH', 'RVEL'], min_members=2)
        with np.errstate(all='ignore'):
            want_q = ES.reduce(rows, quant)
        got = Q.run_pass(ctx, rows, quant, [10, 11])
        assert 'verify' not in got and S.assert_stats(got, want_q, cls + ', quantiles afterwards') == 2 * 3 + 1
    # a pass with a verification that folds no member at all, and one finished without members
    spec = EV.EnsembleVerification(verify=['ZH'], fields=['ZH'])
    zh, y = {'ZH': rows['ZH']}, {'ZH': obs['ZH']}
    empty = ctx.member_verify_fields({}, y, spec, phase=3, n_cells=n_cells, names=('ZH',))
    assert np.isnan(empty['verify']['crps']['ZH']).all() and not empty['verify']['below']['ZH'].any() and not empty['verify']['equal']['ZH'].any()
    assert ctx.member_verify_fields(zh, None, spec, phase=1, capacity=M) is None
    got = ctx.member_verify_fields({}, y, spec, phase=2, n_cells=n_cells, names=('ZH',), capacity=M)
    with np.errstate(all='ignore'):
        assert_result(got, EV.reduce(zh, y, spec), 'finish without members')


# ---------------------------------------------------------------- the refusals
class Hook(C.Structure):
    pass


def raw_hook(ctx, x, phase, change=None, y=None, verify=True, capacity=5, outputs=True, v_outputs=('below', 'equal', 'crps')):
    """cpol_debug_read "member_verify_fields" ("member_stats_fields" with verify=False) on a struct built here: ZH and ZV folded
    (both from x [n_members, n_cells] float32), ZH verified against y; host outputs filled with sentinels; `change(h)` spoils it.
    -> (return code, outputs)"""
    from cosmo_pol_amd import _native as N
    if not hasattr(Hook, '_fields_'):
        Hook._fields_ = [('n_members', C.c_int32), ('n_cells', C.c_int64), ('inp', C.c_void_p * 10), ('ms', N.MemberStats), ('mv', N.MemberVerify)]
    x = np.ascontiguousarray(x, dtype=np.float32)
    n_cells = x.shape[1]
    h = Hook()
    h.n_members, h.n_cells = x.shape
    h.inp[0] = h.inp[1] = x.ctypes.data
    h.ms.phase, h.ms.min_members, h.ms.fields, h.ms.quantile_capacity = phase, 1, 3, capacity
    out = {k: np.full(n_cells, 77, np.float32) for k in ('mean', 'spread', 'crps')}
    out.update({k: np.full(n_cells, 77, np.uint16) for k in ('below', 'equal')})
    out['count'] = np.full((10, n_cells), 77, np.uint16)
    if outputs:
        h.ms.mean[0], h.ms.spread[0], h.ms.count = out['mean'].ctypes.data, out['spread'].ctypes.data, out['count'].ctypes.data
    h.mv.fields, h.mv.fair = 1, 0
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float32)
        h.mv.obs[0] = y.ctypes.data
    for k in v_outputs:
        getattr(h.mv, k)[0] = out[k].ctypes.data
    if change is not None:
        change(h)
    name = b'member_verify_fields' if verify else b'member_stats_fields'
    rc = int(ctx.lib.cpol_debug_read(ctx.h, name, C.byref(h), C.sizeof(h)))      # (the plain hook's struct is the head of this one)
    return rc, out


def untouched(out):
    return all((a == 77).all() for a in out.values())


def test_hook_refusals_leave_the_open_pass_alone():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import ensemble_verify as EV
    ctx = S.ens_op('c2_rsg')._ctx
    rng = np.random.default_rng(9)
    x = S.members_of('random', 5, 129, np.float32, 1, rng)
    y = observations_of(x, 0)
    spec = EV.EnsembleVerification(verify=['ZH'], fields=['ZH', 'ZV'])
    want = EV.reduce({'ZH': x, 'ZV': x}, {'ZH': y}, spec)
    few = x[3:]

    def check_finish(tag):
        rc, out = raw_hook(ctx, few, 2, y=y)
        assert rc == 0, tag
        for k in ('mean', 'spread'):
            assert S.same(out[k], want[k]['ZH']), (tag, k)
        for k in OUT:
            assert S.same(out[k], want['verify'][k]['ZH']), (tag, k)
        assert S.same(out['count'][0], want['count']['ZH']) and (out['count'][2:] == 77).all(), tag

    def s(**kw):
        def change(h):
            for k, v in kw.items():
                if k == 'capacity':
                    h.ms.quantile_capacity = v
                elif k == 'obs':
                    h.mv.obs[0] = v
                else:
                    setattr(h.mv, k, v)
        return change
    # (what is wrong, the phase of the refused call, its members)
    bad = [(s(fields=0), 0, few), (s(fields=0), 1, few), (s(fields=0), 3, few), (s(fields=1 | 1 << 10), 0, few), (s(fields=1 << 31), 1, few),
           # a verified field that the pass does not fold
           (s(fields=1 | 1 << 3), 0, few), (s(fields=1 << 9), 3, few),
           (s(fair=2), 0, few), (s(fair=-1), 1, few), (s(fair=2), 3, few),
           (s(capacity=0), 1, few), (s(capacity=0), 3, few), (s(capacity=0), 0, few),
           # a fold that differs from the open pass: the verified fields, fair
           (s(fields=3), 0, few), (s(fields=2), 2, few), (s(fair=1), 0, few), (s(fair=1), 2, few),
           # beyond the capacity: in the middle of a pass (3 of 5 are folded), in a finishing call, in a call that begins a pass
           (None, 0, x[:3]), (None, 2, x[:3]), (None, 1, np.zeros((6, 129), np.float32)), (None, 3, np.zeros((6, 129), np.float32)),
           # a finishing call without the observations of a verified field
           (s(obs=None), 2, few), (s(obs=None), 3, few)]
    for i, (change, phase, rows) in enumerate(bad):
        assert raw_hook(ctx, x[:3], 1)[0] == 0
        rc, out = raw_hook(ctx, rows, phase, change, y=y)
        assert rc == N.ERR_ARG, (i, phase, rc)
        assert untouched(out), i
        check_finish('after refusal %d' % i)
    # a finishing call with no verify output pointer at all for a verified field (the statistics' pointers do not make up for it)
    assert raw_hook(ctx, x[:3], 1)[0] == 0
    rc, out = raw_hook(ctx, few, 2, y=y, v_outputs=())
    assert rc == N.ERR_ARG and untouched(out)
    check_finish('after a finishing call without verify outputs')
    # ... while one of the three is enough, and the statistics' pointers may all be missing
    assert raw_hook(ctx, x[:3], 1)[0] == 0
    rc, out = raw_hook(ctx, few, 2, y=y, outputs=False, v_outputs=('equal',))
    assert rc == 0 and S.same(out['equal'], want['verify']['equal']['ZH'])
    assert all((out[k] == 77).all() for k in ('mean', 'spread', 'count', 'below', 'crps'))
    # a call of a pass begun with the struct that leaves it out: refused, the pass stays open and finishes
    assert raw_hook(ctx, x[:3], 1)[0] == 0
    for phase in (0, 2):
        rc, out = raw_hook(ctx, few, phase, verify=False)
        assert rc == N.ERR_ARG and untouched(out), phase
    check_finish('after a call without the struct')
    # a call that presents the struct to a pass begun without it: refused, the plain pass stays open and finishes
    assert raw_hook(ctx, x[:3], 1, verify=False)[0] == 0
    for phase in (0, 2):
        rc, out = raw_hook(ctx, few, phase, y=y)
        assert rc == N.ERR_ARG and untouched(out), phase
    rc, out = raw_hook(ctx, few, 2, verify=False)
    assert rc == 0 and S.same(out['mean'], want['mean']['ZH']) and S.same(out['count'][1], want['count']['ZV'])
    assert all((out[k] == 77).all() for k in OUT)
    # the wrapper reports the library's words, and the next valid pass is correct
    both = {'ZH': x, 'ZV': x}
    assert ctx.member_verify_fields({k: v[:3] for k, v in both.items()}, None, spec, phase=1, capacity=5) is None
    with pytest.raises(ValueError, match='cpol_member_verify: fields or fair differ'):
        ctx.member_verify_fields({k: v[3:] for k, v in both.items()}, {'ZH': y}, EV.EnsembleVerification(verify=['ZH'], fair=True, fields=['ZH', 'ZV']),
                                 phase=2, capacity=5)
    with np.errstate(all='ignore'):
        assert_result(ctx.member_verify_fields({k: v[3:] for k, v in both.items()}, {'ZH': y}, spec, phase=2, capacity=5), want, 'wrapper')
    with pytest.raises(ValueError, match='quantile_capacity'):
        ctx.member_verify_fields({'ZH': x, 'ZV': x}, {'ZH': y}, spec, capacity=4)
    with np.errstate(all='ignore'):
        assert_result(ctx.member_verify_fields({'ZH': x, 'ZV': x}, {'ZH': y}, spec), want, 'at the end')


# ---------------------------------------------------------------- end to end
def v_spec(**kw):
    from cosmo_pol_amd import ensemble_stats as ES
    from cosmo_pol_amd import ensemble_verify as EV
    return EV.EnsembleVerification(verify=('ZH', 'RVEL'), quantiles={'ZH': [0.5]}, extremes=True, exceed={'ZH': [ES.dbz(0.0), ES.dbz(20.0)]},
                                   min_members=2, **kw)


def observed(full, names):
    """member 1's field times 1.3, every seventh gate NaN, every eleventh a member's own value"""
    obs = {}
    for j, k in enumerate(names):
        y = (full[k][1] * full[k].dtype.type(1.3)).astype(full[k].dtype)
        flat = y.reshape(-1)
        flat[::7] = np.nan
        flat[::11] = full[k][j % 3].reshape(-1)[::11]
        obs[k] = y
    return obs


@pytest.mark.parametrize('fair', [False, True])
def test_end_to_end(fair):
    import torch
    from cosmo_pol_amd import ensemble_verify as EV
    name = 'c2_rsg'
    op = S.ens_op(name)
    _, _, _, az, el = E.case(name)
    full = op.simulate_rays_ensemble(az, el, form='shared')
    full = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in full.items()}
    assert 'RVEL' in full
    shape = full['ZH'].shape[1:]
    obs = observed(full, ('ZH', 'RVEL'))
    spec = v_spec(fair=fair)
    with np.errstate(all='ignore'):
        want = EV.reduce(full, obs, spec)
    w = want['verify']
    assert w['crps']['ZH'].shape == shape and w['crps']['RVEL'].dtype == np.float64 and w['below']['ZH'].dtype == np.uint16
    assert np.isfinite(w['crps']['ZH']).any() and np.isnan(w['crps']['ZH']).any() and w['equal']['ZH'].any() and w['below']['ZH'].any()
    for form in ('shared', 'per_member'):
        tag = '%s/%s/fair %d' % (name, form, fair)
        # blocking
        got = op.simulate_rays_ensemble_verify(az, el, spec, obs, form=form)
        assert 'ZH' not in got and got['stats']['n_members'] == 3 and set(got['stats']) == set(want)
        assert_result(got['stats'], want, tag)
        for k in S.GEOM:
            assert S.same(got[k], full[k]), (form, k)
        # page-locked buffers on another lane: the one-copy window
        got = op.simulate_rays_ensemble_verify(az, el, spec, obs, form=form, lane=1, pinned=True)
        op.wait(1)
        assert_result(got['stats'], want, tag + '/pinned on lane 1')
        # device observations and device outputs (the statistics' own pointers stay NULL)
        d_obs = {k: torch.from_numpy(v).to('cuda') for k, v in obs.items()}
        dev = {kind: {k: torch.full(shape, 7, dtype={'crps': torch.float64 if k == 'RVEL' else torch.float32}.get(kind, torch.int16),
                                    device='cuda') for k in obs} for kind in OUT}
        ptrs = {kind: {k: a.data_ptr() for k, a in d.items()} for kind, d in dev.items()}
        ptrs['obs'] = {k: a.data_ptr() for k, a in d_obs.items()}
        res = op.simulate_rays_ensemble_verify(az, el, spec, form=form, lane=1, device_outputs={'stats': ptrs})
        op.wait(1)
        assert 'ZH' not in res
        for kind in OUT:
            for k, a in dev[kind].items():
                g = a.cpu().numpy()
                assert S.same(g.view(np.uint16) if kind != 'crps' else g, w[kind][k]), (tag, 'device outputs', kind, k)
    # a budget that cuts the members into three chunks: the observations go with the last
    try:
        op.sequence_memory_budget = 1
        got = op.simulate_rays_ensemble_verify(az, el, spec, obs, form='shared')
        assert_result(got['stats'], want, name + '/one member per chunk')
    finally:
        op.sequence_memory_budget = None
    if fair:
        return
    # the member order does not matter to the three outputs
    got = op.simulate_rays_ensemble_verify(az, el, spec, obs, members=[2, 0, 1])['stats']
    for kind in OUT:
        for k in obs:
            assert S.same(got['verify'][kind][k], want['verify'][kind][k]), (kind, k)
    # a verification alone: no quantiles, one field
    lean = EV.EnsembleVerification(verify=['ZH'], mean=False, spread=False, fields=['ZH'])
    got = op.simulate_rays_ensemble_verify(az, el, lean, {'ZH': obs['ZH']})['stats']
    assert set(got) == {'count', 'exceed', 'verify', 'n_members'}
    with np.errstate(all='ignore'):
        assert_result(got, EV.reduce(full, obs, lean), name + '/lean')


def test_the_calls_around_the_refusals_of_the_sweep_and_the_scan():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import ensemble_stats as ES
    from cosmo_pol_amd import ensemble_verify as EV
    name = 'c2_rsg'
    op = S.ens_op(name)
    ctx = op._ctx
    _, _, _, az, el = E.case(name)
    spec = v_spec()
    full = op.simulate_rays_ensemble(az, el, form='shared')
    full = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in full.items()}
    obs = observed(full, ('ZH', 'RVEL'))
    with np.errstate(all='ignore'):
        want = EV.reduce(full, obs, spec)
    # the calls around it are what they are without it: a plain pass, a pass with quantiles
    op.simulate_rays_ensemble_verify(az, el, spec, obs)
    for other in (S.stats_spec(), Q.q_spec()):
        with np.errstate(all='ignore'):
            S.assert_stats(op.simulate_rays_ensemble_stats(az, el, other)['stats'], ES.reduce(full, other), 'afterwards')
    # the operator's refusals: before anything runs
    ran = []
    orig = op._run_rays
    op._run_rays = lambda *a, **kw: ran.append(1) or orig(*a, **kw)
    try:
        for bad in (None, {'ZH': obs['ZH']}, dict(obs, ZH=obs['ZH'].astype(np.float64)), dict(obs, RVEL=obs['RVEL'][:, :-1]),
                    dict(obs, ZH=obs['ZH'].reshape(-1))):
            with pytest.raises(ValueError, match='observations'):
                op.simulate_rays_ensemble_verify(az, el, spec, bad)
        with pytest.raises(ValueError, match='EnsembleVerification'):       # observations without a verification
            op.simulate_rays_ensemble_verify(az, el, S.stats_spec(), obs)
        with pytest.raises(ValueError, match='observations'):               # a verification without observations
            op.simulate_rays_ensemble_stats(az, el, spec)
        with pytest.raises(ValueError, match='observations'):
            op.get_PPI_ensemble_stats([el[0]], spec, azimuths=az[:2])
        with pytest.raises(ValueError, match='verification: at most 128'):
            op.simulate_rays_ensemble_verify(az, el, EV.EnsembleVerification(), obs, members=list(range(129)))
    finally:
        del op._run_rays
    assert not ran
    # the library's refusals of a sweep: the struct without member_stats, and superobservations in the same call -- nothing is
    # queued, and the next pass is correct
    for spoil in ('no member_stats', 'superob'):
        so = N.Superob()                        # (a valid request of its own: one gate per window, ZH; never written -- the call is refused)
        so.ray_window = so.gate_window = 1
        so.min_valid_fraction = 0.5
        so_zh = np.full(full['ZH'].shape, 77, np.float32)
        so.ZH = so_zh.ctypes.data
        calls = []

        def spy(p, t, members, o, spoil=spoil, so=so, calls=calls):
            assert o.member_verify and o.member_stats
            if spoil == 'superob':
                o.superob = C.pointer(so)
            else:
                o.member_stats = None
            calls.append(1)
            return N.Context.run_sweep_members(ctx, p, t, members, o)
        ctx.run_sweep_members = spy
        try:
            with pytest.raises(ValueError, match='member_verify|member_stats'):
                op.simulate_rays_ensemble_verify(az, el, spec, obs, form='shared')
        finally:
            del ctx.run_sweep_members
        assert calls == [1] and (so_zh == 77).all()
        got = op.simulate_rays_ensemble_verify(az, el, spec, obs, form='shared')
        assert_result(got['stats'], want, 'after the refusal: ' + spoil)
    # a PPI of two sweeps over two lanes, one dict of observations per sweep
    op2 = S.ens_op(name, lanes=2)
    azimuths = az[0] + 0.5 * np.arange(3)
    elevations = [el[0], el[0] + 0.7]
    fulls = [S.reference(op2, azimuths, np.full(3, e), spec, members=[1, 2, 0])[1] for e in elevations]
    obss = [observed(f, ('ZH', 'RVEL')) for f in fulls]
    scans = op2.get_PPI_ensemble_verify(elevations, spec, obss, azimuths=azimuths, members=[1, 2, 0])
    assert len(scans) == 2
    for e, res, f, y in zip(elevations, scans, fulls, obss):
        with np.errstate(all='ignore'):
            assert_result(res['stats'], EV.reduce(f, y, spec), 'PPI at %.1f' % e)
    with pytest.raises(ValueError, match='one dict per sweep'):
        op2.get_PPI_ensemble_verify(elevations, spec, obss[:1], azimuths=azimuths)
