"""Host-side pieces of the time-interpolated scans (cosmo_pol_amd/timeline.py) and the ctypes mirror of the fields that
switch the mode on: no GPU."""
import ctypes
import datetime

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import timeline as TL

SERIES = [0.0, 600.0, 1500.0]


def test_bracket_on_between_and_at_the_last_state():
    lo, w = TL.bracket(SERIES, [0.0, 150.0, 600.0, 1050.0, 1500.0])
    assert lo.dtype == np.int32 and w.dtype == np.float32
    assert lo.tolist() == [0, 0, 1, 1, 2]
    assert w.tolist() == [0.0, 0.25, 0.0, 0.5, 0.0]
    lo, w = TL.bracket(SERIES, 150.0)                      # a scalar keeps its shape
    assert lo.shape == () and int(lo) == 0 and float(w) == 0.25
    assert np.all((w >= 0) & (w < 1))


def test_bracket_weight_is_the_float64_quotient_rounded_once():
    s = [0.1, 0.7, 1.9]
    t = np.array([0.3, 0.1 + 0.6 / 3.0, 1.234567, 0.7000001])
    lo, w = TL.bracket(s, t)
    for i in range(len(t)):
        a, b = s[int(lo[i])], s[int(lo[i]) + 1]
        q = (np.float64(t[i]) - np.float64(a)) / (np.float64(b) - np.float64(a))
        assert w[i].tobytes() == np.float32(q).tobytes(), i
        # (not the float32 quotient of float32 operands)
    q32 = (np.float32(t[2]) - np.float32(0.7)) / (np.float32(1.9) - np.float32(0.7))
    assert isinstance(q32, np.float32)


def test_bracket_a_quotient_that_rounds_to_one_takes_the_later_state():
    t = np.nextafter(600.0, 0.0)                           # (600 - 2^-43) / 600 rounds to 1.0f
    assert np.float32(t / 600.0) == np.float32(1.0)
    lo, w = TL.bracket(SERIES, t)
    assert int(lo) == 1 and float(w) == 0.0


@pytest.mark.parametrize('t', [-1e-9, 1500.0000001, np.nan, [10.0, 2000.0]])
def test_bracket_refuses_times_outside_the_series(t):
    with pytest.raises(ValueError, match='outside the series'):
        TL.bracket(SERIES, t)


def test_bracket_names_the_offending_time():
    with pytest.raises(ValueError, match='1777'):
        TL.bracket(SERIES, [10.0, 1777.0])


@pytest.mark.parametrize('series', [[0.0, 600.0, 600.0], [0.0, 700.0, 600.0], [5.0], [0.0, np.nan, 3.0]])
def test_bracket_refuses_a_series_that_does_not_increase_strictly(series):
    with pytest.raises(ValueError):
        TL.bracket(series, 1.0)


def test_as_seconds_takes_datetimes():
    t0 = datetime.datetime(2024, 6, 1, 12, 0, 0)
    s = TL.as_seconds([t0, t0 + datetime.timedelta(minutes=10)])
    assert s.dtype == np.float64 and s[1] - s[0] == 600.0
    d = TL.as_seconds(np.array(['2024-06-01T12:00:00', '2024-06-01T12:10:00'], dtype='datetime64[s]'))
    assert np.array_equal(d, s)
    lo, w = TL.bracket(s, TL.as_seconds(t0 + datetime.timedelta(minutes=2, seconds=30)))
    assert int(lo) == 0 and float(w) == 0.25


def _states():
    rng = np.random.default_rng(7)
    a = {'T': rng.normal(270, 10, (3, 4, 5)).astype(np.float32), 'U': rng.normal(0, 5, (3, 4, 5)).astype(np.float32)}
    b = {k: (v + rng.normal(0, 1, v.shape)).astype(np.float32) for k, v in a.items()}
    return a, b


def test_blend_states_weight_zero_returns_the_earlier_states_bits():
    a, b = _states()
    a['U'][0, 0, 0] = -0.0
    a['U'][0, 0, 1] = np.nan
    b['U'][0, 0, 2] = np.nan                               # (not read)
    b['U'][0, 0, 3] = -9999.0                              # (not read)
    out = TL.blend_states(a, b, 0.0)
    for k in a:
        assert out[k].dtype == np.float32 and out[k] is not a[k]
        assert out[k].tobytes() == a[k].tobytes(), k
    assert np.signbit(out['U'][0, 0, 0])


def test_blend_states_is_three_float32_operations():
    a, b = _states()
    w = np.float32(1.0 / 3.0)
    out = TL.blend_states(a, b, w)
    for k in a:
        assert out[k].dtype == np.float32
        d = (b[k] - a[k]).astype(np.float32)
        p = (w * d).astype(np.float32)
        want = (a[k] + p).astype(np.float32)
        assert out[k].tobytes() == want.tobytes(), k
    # ... which is not the float64 blend rounded once, somewhere
    rng = np.random.default_rng(11)
    x = {'U': rng.normal(0, 5, 4096).astype(np.float32)}
    y = {'U': rng.normal(0, 5, 4096).astype(np.float32)}
    got = TL.blend_states(x, y, w)['U']
    wide = (x['U'].astype(np.float64) + np.float64(w) * (y['U'].astype(np.float64) - x['U'].astype(np.float64))).astype(np.float32)
    assert (wide != got).any()


def test_blend_states_keeps_the_sentinel_from_either_side_and_propagates_nan():
    a, b = _states()
    a['T'][0, 0, 0] = -9999.0
    b['T'][0, 0, 1] = -9999.0
    a['T'][0, 0, 2] = np.nan
    b['T'][0, 0, 3] = np.nan
    a['T'][0, 1, 0], b['T'][0, 1, 0] = -9999.0, np.nan
    a['T'][0, 1, 1], b['T'][0, 1, 1] = np.nan, -9999.0
    out = TL.blend_states(a, b, 0.25)['T']
    assert out[0, 0, 0] == -9999.0 and out[0, 0, 1] == -9999.0
    assert np.isnan(out[0, 0, 2]) and np.isnan(out[0, 0, 3])
    assert out[0, 1, 0] == -9999.0 and out[0, 1, 1] == -9999.0
    assert np.isfinite(out[1:]).all() and (out[1:] != -9999.0).all()


def test_blend_states_refuses_bad_weights_and_mismatched_states():
    a, b = _states()
    for w in (1.0, -0.1, np.nan):
        with pytest.raises(ValueError):
            TL.blend_states(a, b, w)
    with pytest.raises(ValueError):
        TL.blend_states(a, {'T': b['T']}, 0.5)


def test_plan_ray_groups_lists_only_the_states_the_rays_need():
    lo = np.array([3, 3, 4, 9, 9], dtype=np.int32)
    w = np.array([0.5, 0.0, 0.0, 0.25, 0.0], dtype=np.float32)
    assert TL.plan_ray_groups(lo, w) == [(0, 5, 3, 8)]
    assert TL.plan_ray_groups(lo, w, max_states=4) == [(0, 3, 3, 2), (3, 5, 9, 2)]
    assert TL.plan_ray_groups([5], [0.0]) == [(0, 1, 5, 1)]
    # every ray once, in order, never more than the limit
    rng = np.random.default_rng(3)
    lo = rng.integers(0, 200, 500).astype(np.int32)
    w = np.where(rng.random(500) < 0.3, 0, 0.5).astype(np.float32)
    groups = TL.plan_ray_groups(lo, w, 64)
    assert groups[0][0] == 0 and groups[-1][1] == 500
    for (a0, a1, first, n), nxt in zip(groups, groups[1:] + [None]):
        assert a1 > a0 and 1 <= n <= 64
        need_hi = lo[a0:a1] + (w[a0:a1] != 0)
        assert lo[a0:a1].min() == first and need_hi.max() == first + n - 1
        if nxt is not None:
            assert nxt[0] == a1


def test_ctypes_mirror_has_the_time_blend_fields_and_they_default_to_off():
    """The fields are per-ray tables: appended to cpol_ray_tables_t (cpol_sweep_params keeps v_res as its last member, which
    tests/test_broadening_cpu.py pins).  tests/test_cabi_cpu.py checks the layout against the header."""
    names = [f for f, _ in N.RayTables._fields_]
    assert names[-4:] == ['ray_state', 'ray_weight', 'time_blend', 'pad_time_']
    assert names.index('ray_state') > names.index('ml_radius')       # appended: nothing before them moved
    assert [f for f, _ in N.SweepParams._fields_][-1] == 'v_res'
    t = N.RayTables()
    assert t.time_blend == 0 and t.pad_time_ == 0 and not t.ray_state and not t.ray_weight
    assert N.RayTables.time_blend.size == 4 and N.RayTables.ray_state.size == ctypes.sizeof(ctypes.c_void_p)
    assert N.RayTables.ray_state.offset % 8 == 0 and ctypes.sizeof(N.RayTables) % 8 == 0
    q = N.RayTables.from_buffer_copy(t)
    q.time_blend = 1
    assert t.time_blend == 0


def test_header_documents_the_mode_where_the_members_call_is_described():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'cosmo_pol_amd.h')) as f:
        h = f.read()
    doc = h[h.index('One scan over MANY members'):h.index('CPOL_API int  cpol_run_sweep_members')]
    assert 'TIME BLEND' in doc and 'replaces in the reference: nothing' in doc and 'CPOL_ERR_ARG' in doc
    for field in ('ray_state', 'ray_weight', 'time_blend'):
        assert field in h[h.index('typedef struct {', h.index('cpol_sweep_params;')):h.index('} cpol_ray_tables_t;')], field


def test_operator_has_the_timed_entry_points_and_keeps_the_old_signatures():
    import inspect
    from cosmo_pol_amd import RadarOperator as R
    assert list(inspect.signature(R.simulate_rays_at).parameters) == [
        'self', 'azimuths', 'elevations', 'times', 'on_device', 'device_outputs', 'apply_sensitivity', 'lane', 'pinned']
    assert list(inspect.signature(R.load_model_series).parameters) == [
        'self', 'states', 'times', 'zlevels', 'proj_info', 'resolution', 'cfilename']
    assert list(inspect.signature(R.get_PPI_at).parameters) == [
        'self', 'elevations', 'times', 'azimuths', 'az_step', 'az_start', 'az_stop']
    assert list(inspect.signature(R.get_RHI_at).parameters)[:3] == ['self', 'azimuths', 'times']
    assert isinstance(R.series_times, property) and R.series_times.fset is None
    assert list(inspect.signature(R.simulate_rays).parameters) == [
        'self', 'azimuths', 'elevations', 'on_device', 'device_outputs', 'apply_sensitivity', 'paths', 'lane', 'pinned']
