"""Network composites without a GPU: the additions to the rule (cosmo_pol_amd/composite.py: the gate plane, the source, plane_xy),
every new refusal in Python and in the host validation header (cosmo_pol_amd/csrc/cpol_comp.h through
tests/c_host/comp_check_network.cpp, built with the address and undefined-behaviour sanitizers and run as a program of its own), the
layout of the state with and without SOURCE, and composite.Maps with a plane.  All comparisons are exact, NaNs positionally
equal."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from cosmo_pol_amd import _native as N
from cosmo_pol_amd import composite as CP
from cosmo_pol_amd import neighbourhood as NB
from cosmo_pol_amd import refraction

from test_composite_cpu import EX, EY, F32, assert_same, full_spec, key, same, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nan, inf = np.nan, np.inf


def radar_xy(dist, az):
    """The radar plane's own coordinates, made on the host: ONE float64 multiplication each."""
    rs, rc = CP.ray_tables(az)
    return dist.astype(np.float64) * rs[:, None], dist.astype(np.float64) * rc[:, None]


def gate_spec(products=('max', 'lowest', 'echo_top'), plane='geographic', **kw):
    if 'echo_top' in products:
        kw.setdefault('thresholds', {'ZH': [-1.0, 0.0, 0.75, 3.0], 'KDP': [0.0]})
    return CP.Composite(['ZH', 'KDP'], EX, EY, products=products, plane=plane, **kw)


# ---------------------------------------------------------------------------------------------------- the gate plane
@pytest.mark.parametrize('hr', [None, (0.0, 2500.0)])
def test_host_made_radar_coordinates_as_a_gate_plane_give_the_radar_plane(hr):
    fields, dist, heights, az = sweep(3, 5, 40, EX, EY, rows=10)
    radar = full_spec(height_range=hr)
    plane = gate_spec(height_range=hr)
    for rpb in (0, 5):
        want = CP.finish(CP.compose(radar, fields, dist, heights, az, rays_per_block=rpb))
        got = CP.finish(CP.compose(plane, fields, None, heights, None, rays_per_block=rpb, gate_xy=radar_xy(dist, az)))
        assert_same(got, want, radar, rpb)
        assert int(want['count']['ZH'].sum()) > 20          # (the comparison is not one of empty maps)


def test_gate_plane_counting_and_edges_by_hand():
    spec = CP.Composite('ZH', [0.0, 1.0, 2.0], [0.0, 1.0], plane='geographic')       # two cells
    x = np.array([[0.0, -0.0, 1.0, 2.0, np.nextafter(2.0, 0.0), -1e-300, nan, 0.5, inf, -inf, 0.5, 1.5]])
    y = np.array([[0.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, nan, 0.5, 0.5, 1.0, np.nextafter(1.0, 0.0)]])
    v = np.arange(1, 13, dtype=F32)[None, :]
    h = np.full((1, 12), 100.0, dtype=F32)
    out = CP.finish(CP.compose(spec, {'ZH': v}, None, h, None, gate_xy=(x, y)))
    # cell 0: gates 0, 1 (-0.0 is on the edge 0.0); cell 1: gates 2, 4, 11; the last edge, NaN and infinities are outside
    assert out['count']['ZH'].tolist() == [[[2, 3]]] and out['values']['ZH']['max'].tolist() == [[[2.0, 12.0]]]
    # dist is not read: NaN distances change nothing
    again = CP.finish(CP.compose(spec, {'ZH': v}, np.full((1, 12), nan, dtype=F32), h, [0.0], gate_xy=(x, y)))
    assert_same(again, out, spec)
    for bad in ((x.astype(F32), y), (x[:, :5], y)):
        with pytest.raises(ValueError, match='gate_xy'):
            CP.compose(spec, {'ZH': v}, None, h, None, gate_xy=bad)


def test_plane_xy_of_the_three_kinds():
    rng = np.random.default_rng(5)
    lats, lons = rng.uniform(45.0, 48.0, (3, 7)), rng.uniform(5.0, 11.0, (3, 7))
    x, y = CP.plane_xy('geographic', lats, lons)
    assert x.dtype == y.dtype == np.float64 and np.array_equal(x, lons) and np.array_equal(y, lats)
    pole = (-43.0, 10.0)
    x, y = CP.plane_xy('model', lats, lons, pole)
    rlat, rlon = refraction.wgs_to_rotated(lats, lons, pole[0], pole[1])
    assert np.array_equal(x, rlon) and np.array_equal(y, rlat) and x.shape == lats.shape
    assert np.abs(y).max() < 3.0 and np.abs(x).max() < 4.0           # (around the rotated equator: the pole is the model's)
    with pytest.raises(ValueError, match='south_pole'):
        CP.plane_xy('model', lats, lons)
    x, y = CP.plane_xy(lambda la, lo: ((lo - 8.0) * 75e3, (la - 46.5).astype(F32)), lats, lons)
    assert np.array_equal(x, (lons - 8.0) * 75e3) and y.dtype == np.float64 and np.array_equal(y, (lats - 46.5).astype(F32).astype(np.float64))
    for bad in ('radar', 'mercator', None):
        with pytest.raises(ValueError, match='plane_xy'):
            CP.plane_xy(bad, lats, lons)
    with pytest.raises(ValueError, match='shape'):
        CP.plane_xy('geographic', lats, lons[:2])
    with pytest.raises(ValueError, match='returned'):
        CP.plane_xy(lambda la, lo: (lo[:1], la), lats, lons)


def test_the_composite_spec_with_a_plane_and_a_source():
    base = full_spec()
    assert base.plane == 'radar' and not base.gate_plane and len(base.key) == 6 and 'plane' not in repr(base)
    assert CP.Composite(['ZH', 'KDP'], EX, EY, products=('max', 'lowest', 'echo_top'), thresholds={'ZH': [-1.0, 0.0, 0.75, 3.0], 'KDP': [0.0]},
                        plane='radar') == base

    def proj(lats, lons):
        return lons, lats
    for plane in ('geographic', 'model', proj):
        s = gate_spec(plane=plane)
        assert s.plane is plane and s.gate_plane and s != base and s.key[:6] == base.key
    assert 'plane=geographic' in repr(gate_spec()) and 'plane=proj' in repr(gate_spec(plane=proj))
    s = gate_spec(products=('source', 'max', 'lowest', 'echo_top'))
    assert s.products == ('max', 'lowest', 'echo_top', 'source') and s.product_mask == 7 | CP.SOURCE_BIT == 23
    assert s.planes('ZH') == ['max', 'height_of_max', 'source_of_max', 'lowest', 'height_of_lowest', 'source_of_lowest',
                              'echo_top_0', 'echo_top_1', 'echo_top_2', 'echo_top_3']
    assert gate_spec(products=('lowest', 'source')).planes('KDP') == ['lowest', 'height_of_lowest', 'source_of_lowest']
    assert CP.shape(s, 'KDP', 6, 3) == (2, 7, 2, 3)
    assert CP.PRODUCTS == ('max', 'lowest', 'echo_top')                  # (bit 8 is no product: 'source' is bit 16)


# ---------------------------------------------------------------------------------------------------- the source
def brute_source(spec, calls, product):
    """Per cell: the smallest source among the counting gates of ALL calls whose packed key equals the extreme over all of them --
    a restatement that knows no order and no state.  calls: [(fields, heights, (x, y), source)]; {field: float32 [cells]}."""
    out = {}
    nx, ny = spec.n_x, spec.n_y
    for k in spec.fields:
        gates = {}
        for fields, heights, (x, y), source in calls:
            v = fields[k]
            for r in range(v.shape[0]):
                for g in range(v.shape[1]):
                    val, h, xx, yy = float(v[r, g]), float(heights[r, g]), float(x[r, g]), float(y[r, g])
                    if val != val or h != h or xx != xx or yy != yy:
                        continue
                    ix = sum(1 for e in spec.x_edges if e <= xx) - 1
                    iy = sum(1 for e in spec.y_edges if e <= yy) - 1
                    if not (0 <= ix < nx and 0 <= iy < ny):
                        continue
                    packed = key(val) << 32 | key(h) if product == 'max' else key(h) << 32 | key(val)
                    gates.setdefault(iy * nx + ix, []).append((packed, source))
        plane = np.full(nx * ny, nan, dtype=F32)
        for cell, lst in gates.items():
            best = (max if product == 'max' else min)(p for p, _ in lst)
            plane[cell] = min(s for p, s in lst if p == best)
        out[k] = plane
    return out


def source_calls(seed=11):
    """Three calls over shared cells: few distinct values and heights and few gates per cell, so the winning state often ties
    across calls, and often a later call holds a greater value than an earlier one and raises the state."""
    rng = np.random.default_rng(seed)
    calls = []
    for i, source in enumerate((2, 0, 1)):
        n_rays, ng = 2 + i, 9
        x = rng.uniform(-2.0, 42.0, (n_rays, ng))
        y = rng.uniform(-32.0, 32.0, (n_rays, ng))
        x[0, 0] = nan
        pool = np.array([0.75, 1.5, 2.25, nan], dtype=F32)
        fields = {k: rng.choice(pool, (n_rays, ng)).astype(F32) for k in ('ZH', 'KDP')}
        heights = rng.choice(np.array([250.0, 1000.0], dtype=F32), (n_rays, ng))
        calls.append((fields, heights, (x, y), source))
    return calls


def fold(spec, calls):
    state = None
    for fields, heights, xy, source in calls:
        state = CP.compose(spec, fields, None, heights, None, state=state, gate_xy=xy, source=source)
    return state


def test_source_is_symmetric_in_the_calls_and_agrees_with_a_brute_force_restatement():
    spec = gate_spec(products=('max', 'lowest', 'echo_top', 'source'))
    calls = source_calls()
    want = CP.finish(fold(spec, calls))
    for order in itertools.permutations(range(3)):
        got = CP.finish(fold(spec, [calls[i] for i in order]))
        assert_same(got, want, spec, order)
    for product in ('max', 'lowest'):
        brute = brute_source(spec, calls, product)
        for k in spec.fields:
            plane = want['values'][k]['source_of_' + product]
            assert same(plane.reshape(-1), brute[k]), (product, k, plane, brute[k])
            assert same(np.isnan(plane), np.isnan(want['values'][k][product]))
    # the maps beside the sources are those of a spec without 'source'
    plain = gate_spec()
    ref = CP.finish(fold(plain, [(f, h, xy, 0) for f, h, xy, _ in calls]))
    for k in plain.fields:
        for p in plain.planes(k):
            assert same(want['values'][k][p], ref['values'][k][p]), (k, p)
        assert same(want['count'][k], ref['count'][k])
    # from the data: in at least one cell the winning MAX state ties across calls (the smaller source wins although another
    # call holds it too), and in at least one a later call raises the state of an earlier one
    ties = raises = 0
    single = [CP.compose(spec, f, None, h, None, gate_xy=xy, source=s)['fields']['ZH']['max'] for f, h, xy, s in calls]
    final = fold(spec, calls)['fields']['ZH']['max']
    for cell in range(spec.n_x * spec.n_y):
        holders = [i for i in range(3) if single[i][cell] == final[cell] and final[cell]]
        ties += len(holders) > 1
        raises += any(0 < single[i][cell] < single[j][cell] for i in range(3) for j in range(i + 1, 3))
    assert ties >= 1 and raises >= 1, (ties, raises)
    srcs = want['values']['ZH']['source_of_max']
    assert len(set(srcs[~np.isnan(srcs)].tolist())) >= 2


def test_source_refusals_in_python():
    with pytest.raises(ValueError, match="'source' needs 'max' or 'lowest'"):
        gate_spec(products=('echo_top', 'source'))
    with pytest.raises(ValueError, match="'source' needs"):
        CP.Composite('ZH', EX, EY, products='source')
    for plane in ('polar', 3, None):
        with pytest.raises(ValueError, match='plane'):
            CP.Composite('ZH', EX, EY, plane=plane)
    spec, plain = gate_spec(products=('max', 'source')), gate_spec(products=('max',))
    f, h, xy, _ = source_calls()[0]
    for bad in (-1, 255, 1000):
        with pytest.raises(ValueError, match='source must lie in 0 ... 254'):
            CP.compose(spec, f, None, h, None, gate_xy=xy, source=bad)
        with pytest.raises(ValueError, match='source must lie in 0 ... 254'):
            CP.Maps(spec).set_plane(xy, 0, bad)
    with pytest.raises(ValueError, match="non-zero source"):
        CP.compose(plain, f, None, h, None, gate_xy=xy, source=1)
    with pytest.raises(ValueError, match="non-zero source"):
        CP.Maps(plain).set_plane(xy, 0, 1)
    CP.compose(spec, f, None, h, None, gate_xy=xy, source=254)
    # a pass keeps its plane and its SOURCE bit: the spec is part of the state
    with pytest.raises(ValueError, match='differ from the state'):
        CP.compose(plain, f, None, h, None, gate_xy=xy, state=CP.compose(spec, f, None, h, None, gate_xy=xy))
    with pytest.raises(ValueError, match='differ from the state'):
        CP.compose(CP.Composite(['ZH', 'KDP'], EX, EY, products=('max',), plane='model'), f, None, h, None, gate_xy=xy,
                   state=CP.compose(plain, f, None, h, None, gate_xy=xy))
    # a source plane has no units to threshold
    for plane in ('source_of_max', 'source_of_lowest'):
        with pytest.raises(ValueError, match='not a plane to score'):
            NB.Fractions(gate_spec(products=('max', 'lowest', 'source')), 'ZH', [1.0], [1], plane=plane)
    assert NB.Fractions(gate_spec(products=('max', 'lowest', 'source')), 'ZH', [1.0], [1], plane='lowest').plane_index == 3


# ---------------------------------------------------------------------------------------------------- the host validation header
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('comp_net') / 'comp_check_network')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c_host', 'comp_check_network.cpp'),
                        '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def run(exe, *calls):
    r = subprocess.run([exe] + list(calls), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls)
    return lines


def parse(line):
    assert line.startswith('ok '), line
    parts = line.split(' | ')
    w = parts[0].split()
    out = {name: int(x) for name, x in zip(w[1::2], w[2::2])}
    out['fields'] = {}
    for p in parts[1:]:
        q = p.split()
        out['fields'][int(q[1])] = dict(zip(q[2::2], (int(x) for x in q[3::2])))
    return out


def test_host_header_refusals(exe):
    cases = {
        'plane=2': 'plane must be', 'plane=-1': 'plane must be',
        'plane=1,gx=0': 'gate_x or gate_y', 'plane=1,gy=0': 'gate_x or gate_y', 'plane=1,gx=0,gy=0,rays=1': 'gate_x or gate_y',
        'plane=0,rays=0': 'ray_sin',
        'source=-1,products=17': 'source must lie in 0 ... 254', 'source=255,products=17': 'source must lie in 0 ... 254',
        'source=1': 'non-zero source without SOURCE', 'source=254,products=7,t0=1': 'non-zero source without SOURCE',
        'products=16': 'SOURCE needs MAX or LOWEST', 'products=20,t0=1': 'SOURCE needs MAX or LOWEST',
        'products=8': 'products must name', 'products=32': 'products must name', 'products=49': 'products must name',
        'plane=1,space=1': 'spaceborne', 'products=17,space=1': 'spaceborne',
    }
    for call, word in cases.items():
        line, = run(exe, call)
        assert line.startswith('refused ') and word in line, (call, line)
    # the gate plane needs no ray tables; the radar plane no gate coordinates; every source up to 254
    for call in ('plane=1,rays=0', 'plane=0,gx=0,gy=0', 'products=17,source=254', 'products=18,source=0', 'products=19,source=7,plane=1'):
        assert run(exe, call)[0].startswith('ok '), call


def test_host_header_pass_keeps_plane_and_source_bit(exe):
    out = run(exe, 'phase=1,plane=1,products=17,source=3', 'phase=0,plane=1,products=17,source=0', 'phase=0,plane=0,products=17',
              'phase=0,plane=1,products=1', 'phase=0,plane=1,products=19', 'phase=0,plane=1,products=17,source=255',
              'phase=2,plane=1,products=17,source=254', 'phase=0,plane=1,products=17')
    assert parse(out[0])['open'] == 1 and parse(out[0])['source'] == 3 and parse(out[1])['open'] == 1
    assert 'plane differs from the open pass' in out[2]
    assert 'products or block count differ' in out[3] and 'products or block count differ' in out[4] and '0 ... 254' in out[5]
    # the refusals left the pass as it was: it finishes, and is closed then
    assert parse(out[6])['open'] == 0 and parse(out[6])['plane'] == 1 and 'no pass open' in out[7]
    # the radar plane likewise
    out = run(exe, 'phase=1', 'phase=0,plane=1', 'phase=2')
    assert 'plane differs' in out[1] and parse(out[2])['open'] == 0


def test_host_header_layout_with_and_without_source(exe):
    # without SOURCE: the plan the existing tests pin (test_composite_cpu.test_host_header_plan_and_rounding), nothing behind it
    p = parse(run(exe, 'rows=12,gates=50,fields=0x9,products=7,rpb=3,nx=3,ny=1,t0=2,t3=1')[0])
    per = 12
    f0, f3 = p['fields'][0], p['fields'][3]
    assert (f0['max'], f0['count'], f0['top'], f3['max'], f3['count'], f3['top']) == (0, per * 8, per * 16, per * 24, per * 32, per * 40)
    assert p['zero'] == per * 44 and (f0['low'], f3['low']) == (per * 44, per * 52) and p['state'] == per * 60 == p['total']
    assert (p['scratch'], p['with_source'], f0['src_max'], f0['src_low'], f3['src_max'], f3['src_low']) == (-1, 0, -1, -1, -1, -1)
    assert (f0['planes'], f3['planes']) == (6, 5)
    spec = CP.Composite(['ZH', 'KDP'], np.arange(4.0), [0.0, 1.0], products=('max', 'lowest', 'echo_top'), thresholds={'ZH': [1.0, 2.0], 'KDP': [1.0]})
    assert CP.state_bytes(spec, 4) == p['total']
    # with SOURCE: the same offsets, then a byte per (block, cell), field and product (padded to 8), then the scratch state
    q = parse(run(exe, 'rows=12,gates=50,fields=0x9,products=23,rpb=3,nx=3,ny=1,t0=2,t3=1,plane=1')[0])
    for k in (0, 3):
        for name in ('max', 'count', 'top', 'low'):
            assert q['fields'][k][name] == p['fields'][k][name]
    assert (q['zero'], q['state'], q['with_source']) == (p['zero'], p['state'], 1)
    pad = (per + 7) // 8 * 8
    g0, g3 = q['fields'][0], q['fields'][3]
    assert (g0['src_max'], g0['src_low'], g3['src_max'], g3['src_low']) == (per * 60, per * 60 + pad, per * 60 + 2 * pad, per * 60 + 3 * pad)
    assert q['scratch'] == per * 60 + 4 * pad and q['total'] == 2 * per * 60 + 4 * pad and (g0['planes'], g3['planes']) == (8, 7)
    spec_s = CP.Composite(['ZH', 'KDP'], np.arange(4.0), [0.0, 1.0], products=('max', 'lowest', 'echo_top', 'source'),
                          thresholds={'ZH': [1.0, 2.0], 'KDP': [1.0]}, plane='geographic')
    assert CP.state_bytes(spec_s, 4) == q['total']
    # LOWEST alone with SOURCE, an odd cell count: one byte array, padded
    r = parse(run(exe, 'rows=1,fields=0x4,products=18,nx=3,ny=3')[0])
    assert (r['state'], r['fields'][2]['src_max'], r['fields'][2]['src_low'], r['scratch'], r['total']) == (144, -1, 144, 160, 304)
    assert CP.state_bytes(CP.Composite('ZDR', np.arange(4.0), np.arange(4.0), products=('lowest', 'source')), 1) == 304
    # the 1 GiB limit counts what SOURCE adds: 1023 x 1023 cells, MAX + LOWEST, 3 fields, 13 blocks fit without (979 MB), not with
    big = 'rows=13,rpb=1,fields=0x7,nx=1023,ny=1023,products=%d'
    assert run(exe, big % 3)[0].startswith('ok ')
    line, = run(exe, big % 19)
    assert line.startswith('refused ') and '1 GiB' in line
    small = parse(run(exe, 'rows=6,rpb=1,fields=0x7,nx=1023,ny=1023,products=19')[0])
    assert small['total'] <= 1 << 30
    spec_b = CP.Composite(['ZH', 'ZV', 'ZDR'], np.arange(1024.0), np.arange(1024.0), products=('max', 'lowest', 'source'))
    assert CP.state_bytes(spec_b, 6) == small['total'] and CP.state_bytes(spec_b, 13) > CP.MAX_STATE_BYTES


# ---------------------------------------------------------------------------------------------------- the struct and the product
def test_struct_carries_plane_source_and_version():
    spec = gate_spec(products=('max', 'source'))
    x, y = np.arange(8.0).reshape(2, 4), -np.arange(8.0).reshape(2, 4)
    c, keep = N.Context.composite_struct(spec, phase=1, gate_xy=(x, y), source=7, plane_version=99)
    assert (c.plane, c.source, c.plane_version, c.products) == (1, 7, 99, 17) and c.gate_x == x.ctypes.data and c.gate_y == y.ctypes.data
    assert not c.ray_sin and not c.ray_cos and any(a is x for a in keep) and any(a is y for a in keep)
    c, _ = N.Context.composite_struct(full_spec(), azimuths=[0.0])
    assert (c.plane, c.source, c.plane_version) == (0, 0, 0) and not c.gate_x and not c.gate_y and c.ray_sin
    with pytest.raises(ValueError, match='differ in shape'):
        N.Context.composite_struct(spec, gate_xy=(x, y[:1]))


def test_maps_with_a_plane_attach_and_bind():
    spec = gate_spec(products=('max', 'lowest', 'source'))
    az = np.arange(4.0)
    x, y = np.arange(20.0).reshape(4, 5), np.ones((4, 5))
    p = CP.Maps(spec, keep_gates=False, phase=3, rays_per_block=2)
    host = lambda block: None       # noqa: E731  (host outputs: attach is handed the block allocator; a composite takes no block)
    with pytest.raises(ValueError, match='needs the per-gate coordinates'):
        p.attach(N, az, 5, None, True, True, ['U'], host)
    p.set_plane((x, y), 41, 2)
    structs, keep = p.attach(N, az, 5, None, True, True, ['U'], host)
    c = structs['composite']
    assert (c.plane, c.source, c.plane_version, c.products) == (1, 2, 41, 3 | CP.SOURCE_BIT) and c.gate_x == x.ctypes.data and c.gate_y == y.ctypes.data
    assert not c.ray_sin and not c.ray_cos
    assert p.arrays() == [('ZH', F32, (2, 6, 2, 3)), ('KDP', F32, (2, 6, 2, 3)), ('count', np.uint64, (2, 2, 2, 3))]
    for i, (path, _, _) in enumerate(p.arrays()):
        p.bind(path, 0x1000 * (i + 1))
    assert c.values[0] == 0x1000 and c.values[3] == 0x2000 and c.count == 0x3000
    # the members of an ensemble call share the geometry: the coordinates stay [n_rays, n_gates]
    p.attach(N, az, 5, 3, True, True, ['U'], host)
    assert p.n_rows == 12
    with pytest.raises(ValueError, match=r'gate_xy: two arrays \[n_rays, n_gates\]'):
        p.attach(N, az[:2], 5, None, True, True, ['U'], host)
    # set anew between the calls of a pass, like the phase
    p.set_plane((x + 1.0, y), 42, 0)
    p.phase = 0
    c = p.attach(N, az, 5, None, True, True, ['U'], host)[0]['composite']
    assert (c.source, c.plane_version, c.phase) == (0, 42, 0) and p.arrays() == []
    # device outputs: the caller's device pointers
    p.phase = 3
    p.set_plane(None, 0, 1)
    c = p.attach(N, az, 5, None, True, True, ['U'], None)[0]['composite']
    assert c.plane == 1 and not c.gate_x
    p.bind_device({'gate_x': 7, 'gate_y': 9, 'count': 11})
    assert (c.gate_x, c.gate_y, c.count, c.source) == (7, 9, 11, 1)
    # the radar plane is what it was
    q = CP.Maps(full_spec())
    c = q.attach(N, az, 5, None, True, True, ['U'], host)[0]['composite']
    assert (c.plane, c.source) == (0, 0) and c.ray_sin and not c.gate_x
    # a scoring product hands the plane through
    s = NB.Scores(NB.Fractions(spec, 'ZH', [1.0], [1]), np.zeros((2, 3), F32), phase=1)
    s.set_plane((x, y), 5, 3)
    c = s.attach(N, az, 5, None, True, True, ['U'], host)[0]['composite']
    assert (c.plane, c.source, c.plane_version) == (1, 3, 5)
