"""Spectrum moments on the GPU (k_spec_moments, cpol_spectrum.inl) against the NumPy statement of the rule
(cosmo_pol_amd/spectrum_moments.py), BIT FOR BIT: NaN where the rule has NaN, identical bits everywhere else, `count` equal.
The kernel alone through the test hook on chosen rows and on the committed spectra; through the sweep in every output mode;
every refusal; the scans."""
import copy
import ctypes as C

import numpy as np
import pytest

import _broadening as B
import _cases
from cosmo_pol_oracle import config as ocfg

pytestmark = pytest.mark.gpu

N_V = (1, 2, 63, 64, 65, 127, 128, 129, 257, 2049, 4097)
N_ROWS = (1, 3, 130)
SPECTRA = ('radial_d3_turb_motion_fft256', 'radial_d3_turb_masked', 'radial_d3_melt')
SWEEPS = ('d3_turb_motion_sub', 'd3_turb_motion_fft256')
SENTINEL = -12345.678


def SM():
    from cosmo_pol_amd import spectrum_moments
    return spectrum_moments


def assert_same_bits(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != 'f':
        assert np.array_equal(got, want), what
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, int((np.isnan(got) != nan).sum()))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    a, b = np.ascontiguousarray(got).view(u)[~nan], np.ascontiguousarray(want).view(u)[~nan]
    assert np.array_equal(a, b), (what, int((a != b).sum()), a.size)


def assert_moments_equal(got, want, fields, what=''):
    assert set(got) == set(want) == set(fields) | {'count'}, (what, sorted(got), sorted(want))
    assert got['count'].dtype == np.uint16
    assert np.array_equal(got['count'], want['count']), what
    for k in fields:
        assert_same_bits(got[k], want[k], (what, k))


def chosen_rows(n_rows, n_v, rng):
    """Rows of every kind the kernel can go wrong on, kind = row index modulo their number; with fewer rows than kinds the
    first kinds.  Bins that exist only in longer rows are skipped."""
    S = rng.random((n_rows, n_v)) + 0.05
    last = n_v - 1
    for i in range(n_rows):
        kind = i % 12
        if kind == 1:                                   # NaN bins at the lane boundaries
            for v in (0, 63, 64, last):
                if v < n_v:
                    S[i, v] = np.nan
        elif kind == 2:                                 # no counting bin: NaN, zeros, -0.0, negative
            S[i] = np.resize(np.array([np.nan, 0.0, -0.0, -1.0]), n_v)
        elif kind == 3:                                 # one counting bin, in the last round of its lane
            S[i] = 0.0
            S[i, last - (last % 64) // 2] = 3.25
        elif kind == 4:                                 # all bins equal
            S[i] = 0.7
        elif kind == 5:                                 # the peak in the last bin
            S[i, last] = 9.0
        elif kind == 6:                                 # a tie between bin 63 and bin 64 (else between the first and the last bin)
            a, b = (63, 64) if n_v > 64 else (0, last)
            S[i, a] = S[i, b] = 5.0
        elif kind == 7:                                 # 1e-300 ... 1e300 in one row: the higher moments overflow
            S[i] = 10.0 ** rng.uniform(-300, 300, n_v)
            S[i, 0] = S[i, last] = 1e300               # (at both ends: the mean lies between them, the fourth moment overflows)
            S[i, n_v // 2] = 1e-300
        elif kind == 8:                                 # the power itself overflows: inf / inf
            S[i, ::2] = 1.7e308
        elif kind == 9:                                 # subnormals alone
            S[i] = rng.integers(1, 1 << 40, n_v).astype(np.float64) * 5e-324
        elif kind == 10:                                # subnormals and zeros beside normal bins, an infinite bin
            S[i, ::3] = 5e-324
            S[i, 1::7] = 0.0
            if n_v > 4:
                S[i, 4] = np.inf
        elif kind == 11:                                # everything censored but bins 0 and the last
            S[i, 1:last] = np.nan
    return S


@pytest.fixture(scope='module')
def ctx():
    from cosmo_pol_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize('n_v', N_V)
def test_hook_against_the_rule(ctx, n_v):
    sm = SM()
    rng = np.random.default_rng(1000 + n_v)
    V = np.linspace(-500.0, 500.0, n_v) if n_v > 1 else np.array([2.5])     # (wide: the fourth moment of a 1e300 bin overflows)
    every = sm.SpectrumMoments(fields=sm.FIELDS)
    picky = sm.SpectrumMoments(fields=sm.FIELDS, min_power=0.3, min_bins=3)
    for n_rows in N_ROWS:
        S = chosen_rows(n_rows, n_v, rng)
        for spec in (every, picky):
            want = sm.moments(S, V, spec)
            got = ctx.spectrum_moments_rows(S, V, spec)
            assert_moments_equal(got, want, sm.FIELDS, (n_v, n_rows, spec))
        if n_rows == 130:                               # (not vacuous: the degenerate gates are there, and inf and NaN arise)
            want = sm.moments(S, V, every)
            assert (want['count'] == 0).any() and (want['count'] == 1).any()
            if n_v >= 63:
                assert np.isinf(want['POWER']).any() and np.isinf(want['KURTOSIS']).any()
                assert np.isnan(want['VMEAN'][want['count'] > 2]).any()


@pytest.mark.parametrize('n_v', (65, 129))
def test_hook_every_field_alone_and_unrequested_rows_untouched(ctx, n_v):
    sm = SM()
    rng = np.random.default_rng(7)
    V = np.linspace(-20.0, 21.0, n_v)
    S = chosen_rows(130, n_v, rng)
    want = sm.moments(S, V, sm.SpectrumMoments(fields=sm.FIELDS))
    for sets in [(k,) for k in sm.FIELDS] + [('VMEAN', 'KURTOSIS', 'VHIGH'), sm.FIELDS]:
        spec = sm.SpectrumMoments(fields=sets)
        out = np.full((8, 130), SENTINEL)
        got = ctx.spectrum_moments_rows(S, V, spec, out=out)
        assert_moments_equal(got, {k: want[k] for k in sets + ('count',)}, sets, sets)
        for r, k in enumerate(sm.FIELDS):
            if k in sets:
                assert_same_bits(out[r], want[k], (sets, k))
            else:
                assert (out[r] == SENTINEL).all(), (sets, k)             # not the caller's to be written: left alone


@pytest.mark.parametrize('name', SPECTRA)
def test_hook_on_the_committed_spectra(ctx, golden, name):
    from test_spectrum_moments_cpu import fixture_varray
    sm = SM()
    g = golden(name)
    V = fixture_varray(g, name)
    for key in ('cutll_DSPECTRUM', 'obs_DSPECTRUM'):
        S = np.ascontiguousarray(g[key], dtype=np.float64)
        for spec in (sm.SpectrumMoments(fields=sm.FIELDS), sm.SpectrumMoments(fields=sm.FIELDS, min_power=float(np.nanmedian(S)), min_bins=5)):
            want = sm.moments(S, V, spec)
            assert_moments_equal(ctx.spectrum_moments_rows(S, V, spec), want, sm.FIELDS, (name, key, spec))
        assert np.isfinite(want['WIDTH']).sum() > 10


def test_hook_refusals_leave_the_context_usable(ctx):
    from cosmo_pol_amd import _native as N
    sm = SM()
    V = np.linspace(-3.0, 3.0, 33)
    S = np.random.default_rng(2).random((5, 33))
    spec = sm.SpectrumMoments(fields=sm.FIELDS)
    want = sm.moments(S, V, spec)
    real = N.Context.spectrum_moments_struct

    def edited(**kw):
        def make(s):
            st = real(s)
            for k, v in kw.items():
                setattr(st, k, v)
            return st
        return staticmethod(make)
    try:
        for kw in (dict(fields=0), dict(fields=1 << 8), dict(fields=0x1FF), dict(min_bins=0), dict(min_bins=-1), dict(min_bins=65536),
                   dict(min_power=-1e-300), dict(min_power=float('nan')), dict(min_power=float('inf'))):
            N.Context.spectrum_moments_struct = edited(**kw)
            with pytest.raises(ValueError):
                ctx.spectrum_moments_rows(S, V, spec)
            N.Context.spectrum_moments_struct = staticmethod(real)
            assert_moments_equal(ctx.spectrum_moments_rows(S, V, spec), want, sm.FIELDS, kw)
    finally:
        N.Context.spectrum_moments_struct = staticmethod(real)
    with pytest.raises(ValueError):
        ctx.spectrum_moments_rows(np.ones((2, 4098)), np.ones(4098), spec)
    with pytest.raises(ValueError):
        ctx.spectrum_moments_rows(np.ones((0, 4)), np.ones(4), spec)
    assert_moments_equal(ctx.spectrum_moments_rows(S, V, spec), want, sm.FIELDS, 'after the shapes')


# ---- through the sweep ----
def _operator(name):
    from cosmo_pol_amd import RadarOperator
    over, az, el, cube, two = B.case_inputs(name)
    conf = ocfg.make_config(over)
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in ocfg.hydrometeor_list(conf)}
    op = RadarOperator(config=copy.deepcopy(over), luts=luts)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    return op, az, el


@pytest.fixture(scope='module', params=SWEEPS)
def sweep(request):
    """(operator, azimuth, elevation, plain simulate_rays result, the rule on its delivered spectrum): made once, never changed"""
    sm = SM()
    op, az, el = _operator(request.param)
    plain = op.simulate_rays([az], [el])
    V = np.ascontiguousarray(op.constants.VARRAY, dtype=np.float64)
    spec = sm.SpectrumMoments(fields=sm.FIELDS, min_bins=2)
    want = sm.moments(plain['DSPECTRUM'], V, spec)
    yield op, az, el, plain, V, spec, want
    op.close()


def _same_arrays(got, want, skip=()):
    for k, v in want.items():
        if k in skip or not isinstance(v, np.ndarray):
            continue
        assert_same_bits(got[k], v, k)


def test_through_the_sweep(sweep):
    sm = SM()
    op, az, el, plain, V, spec, want = sweep
    n_v = len(V)
    assert plain['DSPECTRUM'].shape[1:] == (60, n_v) and n_v in (33, 257)
    assert np.isnan(plain['DSPECTRUM']).any() and np.isfinite(want['WIDTH']).sum() > 10         # (censored bins; not vacuous)
    # keep_spectrum: every array of simulate_rays, and the rule on the delivered spectrum
    res = op.simulate_rays_moments([az], [el], spec, keep_spectrum=True)
    assert set(res) == set(plain) | {'moments'}
    _same_arrays(res, plain)
    assert_moments_equal(res['moments'], sm.moments(res['DSPECTRUM'], V, spec), sm.FIELDS, 'keep')
    assert_moments_equal(res['moments'], want, sm.FIELDS, 'keep, against the plain sweep')
    assert res['moments']['WIDTH'].shape == (1, 60)
    # without: the same bits, no spectrum
    res = op.simulate_rays_moments([az], [el], spec)
    assert 'DSPECTRUM' not in res and set(res) == (set(plain) - {'DSPECTRUM'}) | {'moments'}
    _same_arrays(res, plain, skip=('DSPECTRUM',))
    assert_moments_equal(res['moments'], want, sm.FIELDS, 'no spectrum')
    # a partial field list
    part = sm.SpectrumMoments(fields=('WIDTH', 'VPEAK'), min_bins=2)
    res = op.simulate_rays_moments([az], [el], part)
    assert_moments_equal(res['moments'], {k: want[k] for k in ('WIDTH', 'VPEAK', 'count')}, ('WIDTH', 'VPEAK'), 'partial')
    # pinned, then wait
    for keep in (True, False):
        res = op.simulate_rays_moments([az], [el], spec, keep_spectrum=keep, pinned=True)
        op.wait()
        assert ('DSPECTRUM' in res) == keep
        _same_arrays(res, plain, skip=() if keep else ('DSPECTRUM',))
        assert_moments_equal(res['moments'], want, sm.FIELDS, ('pinned', keep))
    # nothing lingers: the plain sweep afterwards
    again = op.simulate_rays([az], [el])
    assert set(again) == set(plain)
    _same_arrays(again, plain)


def test_through_the_sweep_with_device_outputs(sweep):
    """device pointers: written in place, only the rows asked for"""
    import torch
    sm = SM()
    op, az, el, plain, V, spec, want = sweep
    n_v = len(V)
    n = 60
    mom = torch.full((8, 1, n), SENTINEL, dtype=torch.float64, device='cuda')
    cnt = torch.full((1, n), 77, dtype=torch.int16, device='cuda')
    zh = torch.empty((1, n), dtype=torch.float32, device='cuda')
    sp = torch.empty((1, n, n_v), dtype=torch.float64, device='cuda')
    for fields, with_spectrum in ((sm.FIELDS, True), (('POWER', 'SKEWNESS'), False)):
        mom.fill_(SENTINEL)
        ptrs = {'ZH': zh.data_ptr(), 'moments': {'moments': mom.data_ptr(), 'count': cnt.data_ptr()}}
        if with_spectrum:
            ptrs['DSPECTRUM'] = sp.data_ptr()
        op.simulate_rays_moments([az], [el], sm.SpectrumMoments(fields=fields, min_bins=2), device_outputs=ptrs)
        op.wait()
        rows = mom.cpu().numpy()
        assert np.array_equal(cnt.cpu().numpy().view(np.uint16), want['count'])
        assert_same_bits(zh.cpu().numpy(), plain['ZH'], 'device ZH')
        for r, k in enumerate(sm.FIELDS):
            if k in fields:
                assert_same_bits(rows[r], want[k], ('device', k))
            else:
                assert (rows[r] == SENTINEL).all(), ('device', k)
        if with_spectrum:
            assert_same_bits(sp.cpu().numpy(), plain['DSPECTRUM'], 'device DSPECTRUM')
    # nothing lingers: the plain sweep afterwards
    again = op.simulate_rays([az], [el])
    assert set(again) == set(plain)
    _same_arrays(again, plain)


def _spy_run_sweep(op, call):
    """the structs of the cpol_run_sweep call that `call` makes"""
    ctx, seen = op._ctx, []
    real = ctx.run_sweep
    ctx.run_sweep = lambda p, t, o: (seen.append((p, t, o)), real(p, t, o))[1]
    try:
        call()
    finally:
        del ctx.run_sweep
    assert len(seen) == 1
    return seen[0]


def test_window_rows_and_every_refusal(sweep):
    """The C ABI itself: blocking host arrays, and page-locked arrays under the one-copy window rule (rows of `moments` outside
    `fields` arrive as zeros); then every refusal of the header's list, each followed by a good call with the bits of the
    sweep test."""
    from cosmo_pol_amd import _native as N
    sm = SM()
    op, az, el, plain, V, spec, want = sweep
    ctx = op._ctx
    p, t, _ = _spy_run_sweep(op, lambda: op.simulate_rays([az], [el]))
    n = 60

    def call(mode, edit=None, fields=sm.FIELDS, via=None, with_count=True):
        q = N.SweepParams.from_buffer_copy(p)
        q.outputs_on_device = mode
        if mode == 2:
            slab = ctx.host_alloc(8 * n * 8 + n * 2 + 64)
            slab[:] = 0x5A
            mom, cnt = slab[:8 * n * 8].view(np.float64).reshape(8, n), slab[8 * n * 8:8 * n * 8 + 2 * n].view(np.uint16)
        else:
            mom, cnt = np.full((8, n), SENTINEL), np.full(n, 77, np.uint16)
        st = N.Context.spectrum_moments_struct(sm.SpectrumMoments(fields=fields, min_bins=2))
        st.moments, st.count = mom.ctypes.data, cnt.ctypes.data if with_count else None
        o = N.Outputs()
        o.spectrum_moments = C.pointer(st)
        keep = []
        if edit is not None:
            keep = edit(q, st, o)
        (via or (lambda q, t, o: ctx.run_sweep(q, t, o)))(q, t, o)
        ctx.synchronize()
        del keep
        return mom, cnt

    def good(what):
        mom, cnt = call(0)
        assert np.array_equal(cnt, want['count'].reshape(-1)), what
        for r, k in enumerate(sm.FIELDS):
            assert_same_bits(mom[r], want[k].reshape(-1), (what, k))
    good('blocking host arrays')
    mom, cnt = call(0, with_count=False)
    assert (cnt == 77).all()
    assert_same_bits(mom[2], want['WIDTH'].reshape(-1), 'no count')
    # page-locked arrays: one window; the rows nobody asked for arrive as zeros
    mom, cnt = call(2, fields=('POWER', 'WIDTH', 'VHIGH'))
    assert np.array_equal(cnt, want['count'].reshape(-1))
    for r, k in enumerate(sm.FIELDS):
        if k in ('POWER', 'WIDTH', 'VHIGH'):
            assert_same_bits(mom[r], want[k].reshape(-1), ('window', k))
        else:
            assert (mom[r].view(np.uint64) == 0).all(), ('window', k)
    # blocking host arrays: the rows nobody asked for are left alone
    mom, cnt = call(0, fields=('VMEAN',))
    assert (mom[[0, 2, 3, 4, 5, 6, 7]] == SENTINEL).all()
    assert_same_bits(mom[1], want['VMEAN'].reshape(-1), 'one row')

    so_out = np.zeros(n, np.float32)

    def with_superob(q, st, o):
        so = N.Superob()
        so.ray_window, so.gate_window, so.min_valid_fraction, so.ZH = 1, 2, 0.5, so_out.ctypes.data
        o.superob = C.pointer(so)
        return [so]

    def with_stats(q, st, o):
        ms = N.MemberStats()
        ms.phase, ms.min_members, ms.fields = 3, 1, 1
        ms.mean[0] = so_out.ctypes.data
        o.member_stats = C.pointer(ms)
        return [ms]
    refusals = [
        ('scheme 1', lambda q, st, o: setattr(q, 'simulate_doppler', 1)),
        ('no Doppler', lambda q, st, o: setattr(q, 'simulate_doppler', 0)),
        ('fields 0', lambda q, st, o: setattr(st, 'fields', 0)),
        ('fields bit 8', lambda q, st, o: setattr(st, 'fields', 0x100 | 1)),
        ('min_bins 0', lambda q, st, o: setattr(st, 'min_bins', 0)),
        ('min_bins 65536', lambda q, st, o: setattr(st, 'min_bins', 65536)),
        ('min_power < 0', lambda q, st, o: setattr(st, 'min_power', -1.0)),
        ('min_power NaN', lambda q, st, o: setattr(st, 'min_power', float('nan'))),
        ('min_power inf', lambda q, st, o: setattr(st, 'min_power', float('inf'))),
        ('moments NULL', lambda q, st, o: setattr(st, 'moments', None)),
        ('superob', with_superob),
        ('member_stats', with_stats),
    ]
    for what, edit in refusals:
        with pytest.raises(ValueError):
            call(0, edit=edit)
        good('after ' + what)
    with pytest.raises(ValueError, match='spectrum moments'):
        call(0, via=lambda q, t, o: ctx.run_sweep_members(q, t, [0], o))
    good('after cpol_run_sweep_members')
    with pytest.raises(ValueError, match='spectrum moments'):
        call(0, via=lambda q, t, o: ctx.run_columns(q, N.Columns(), o))
    good('after cpol_run_columns')
    # the Python layer: ValueError before anything is queued
    submitted = ctx.submitted
    for bad in (None, 'WIDTH', ('WIDTH',), object()):
        with pytest.raises(ValueError):
            op.simulate_rays_moments([az], [el], bad)
    for kw in (dict(fields=()), dict(fields=('ZH',)), dict(min_bins=0), dict(min_power=-1.0), dict(min_power=float('nan'))):
        with pytest.raises(ValueError):
            op.simulate_rays_moments([az], [el], sm.SpectrumMoments(**kw))
    with pytest.raises(ValueError):
        op.simulate_rays_moments([az], [el], spec, device_outputs={'moments': {'WIDTH': 1}})
    assert ctx.submitted == submitted
    res = op.simulate_rays_moments([az], [el], spec)
    assert_moments_equal(res['moments'], want, sm.FIELDS, 'after the Python refusals')


def test_other_doppler_schemes_are_refused_in_python():
    sm = SM()
    over, az, el, cube, two = B.case_inputs('d3_turb_motion_sub')
    over = copy.deepcopy(over)
    over['doppler'].update(scheme=1, turbulence_correction=0, motion_correction=0)
    cube['data'].pop('EDR', None)
    from cosmo_pol_amd import RadarOperator
    conf = ocfg.make_config(over)
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in ocfg.hydrometeor_list(conf)}
    op = RadarOperator(config=over, luts=luts)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    submitted = op._ctx.submitted
    with pytest.raises(ValueError, match='scheme 3'):
        op.simulate_rays_moments([az], [el], sm.SpectrumMoments())
    with pytest.raises(ValueError, match='scheme 3'):
        op.get_PPI_moments([el], sm.SpectrumMoments(), azimuths=[az])
    assert op._ctx.submitted == submitted
    assert np.isfinite(op.simulate_rays([az], [el])['RVEL']).any()
    op.close()


def test_scans(sweep):
    sm = SM()
    op, az, el, plain, V, spec, want = sweep
    azs = [az, az + 1.0, az + 2.0, az + 3.0]
    els = [el, el + 1.0]
    scans = op.get_PPI_moments(els, spec, azimuths=azs, keep_spectrum=True)
    assert len(scans) == 2
    for e, res in zip(els, scans):
        one = op.simulate_rays_moments(azs, [e] * 4, spec, keep_spectrum=True)
        assert res['moments']['WIDTH'].shape == (4, 60)
        assert_moments_equal(res['moments'], one['moments'], sm.FIELDS, ('ppi', e))
        assert_same_bits(res['DSPECTRUM'], one['DSPECTRUM'], 'ppi spectrum')
        assert_moments_equal(res['moments'], sm.moments(res['DSPECTRUM'], V, spec), sm.FIELDS, ('ppi rule', e))
    assert_moments_equal({k: v[:1] for k, v in scans[0]['moments'].items()}, want, sm.FIELDS, 'first ray')
    els3 = [el, el + 1.0, el + 2.0]
    scans = op.get_RHI_moments([az, az + 5.0], spec, elevations=els3)
    assert len(scans) == 2
    for a, res in zip((az, az + 5.0), scans):
        assert 'DSPECTRUM' not in res
        one = op.simulate_rays_moments([a] * 3, els3, spec)
        assert_moments_equal(res['moments'], one['moments'], sm.FIELDS, ('rhi', a))
