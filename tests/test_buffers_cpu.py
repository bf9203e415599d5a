"""The work-buffer plan of a sweep (cosmo_pol_amd/csrc/cpol_buffers.h: plan_buffers, BUF_ROWS, buf_key_list) on the host, through
tests/c_host/buffers_check.cpp.  No expected value here comes from plan_buffers itself: each buffer's size and condition is stated
from the ENSURE lines run_sequence had before the rule moved (cosmo_pol_hip.hip at commit a227de5, line numbers of that file):

  traj       mode == HOST_PATHS or debug reads or f.prep_paths: n_rays * n_v * 3 * n_gates float32              3588-3589
  rayc       f.ray_prep: (n_rays * n_h + n_rays) * 2 float64                                                     3590
  poly       f.geo_poly: n_rays * n_h * 2 * CPOL_GEO_NP float64                                                  3594
  timed      a time-blended call: 2 * n_rays int32                                                               3634-3636
  vals mask elev qmelt fwmelt     always: n_vars * 4, 1, 4, 2 * 4, 2 * 8 bytes per sub-beam gate                 3654-3656, 3659-3660
  coords     debug reads: 2 float32 per sub-beam gate                                                            3657
  wgate      integration scheme 'ml': float64 per sub-beam gate                                                  3658
  key pos par rec perm res        always, per species and sub-beam gate: 4, 4, CPOL_MAX_PAR * 8, 16, 4, CPOL_N_SZ * 8
                                                                                                                 3661-3663, 3685, 3690-3691
  count      2 sets of cnt_stride = n_keys + 3 + CPOL_COUNT_SLOTS int32; totals 2 * 4 int64                      3665, 3669-3670
  blkranked  ceil(n_sbg / CPOL_CLASSIFY_THREADS) int32; vmask 1 byte per sub-beam gate; offset 2 * n_keys int32  3684, 3686-3687
  vn icefirst proj                Doppler: 2 float64 per item; sizeof(IceFirst) = 24 per (ray, sub-beam); f.rvel_terms: float64
                                  per sub-beam gate                                                              3692-3696
  colin      columns with host inputs: every input padded to 256 bytes -- the variables float32, then mask int8, elev float32,
             wgate float64, q_melt 2 float32, fw_melt 2 float64 per sub-beam gate, has_melting 1 byte per (ray, sub-beam), an
             input that is not given 0 bytes; the copies go to the running padded sum                            3703-3715, 3894-3903
  xscr xgeo  sub-beam export, xa8 / xa4 / xa1 = 8 / 4 / 1 bytes per sub-beam gate padded to 256: n_vars * xa4 + xa1 + xa4 with the
             mask behind the values and the elevation behind the mask; 2 * xa8 + 3 * xa4 + xa1 with lats, lons, dist, heights,
             elev, mask_ml in turn                                                                               3719-3724, 3982-3996
  beam       Doppler scheme 3: n_vbins float32 per sub-beam gate; with broadening bsigma float64 per sub-beam gate and bon int32
             per (ray, sub-beam)                                                                                 3725-3731
  gscan defer   f.gate1: 3 float32 and 1 byte per gate                                                           3735-3738
  present    f.gate1_ray in a build with CPOL_GATE1_PRESENT: n_rays * ceil(n_gates / 64) words                   3739-3745
  ticket     f.gate1_ray and f.g1r == 3: n_rays int32                                                            3746-3751
  units      unless f.rare_direct: unit_cap = n_hyd * n_sbg / 64 + n_keys + 64 WorkUnit of 16 bytes; with it unit_cap =
             n_hyd * n_sbg and no buffer                                                                         3689, 3752-3753
  szinteg    debug reads or f.subsum: n_rg * n_hyd * CPOL_N_SZ float32                                           3754-3755
  clk        debug reads, in the PSD stage, which the sub-beam export never reaches: 2048 * 4 int64             4020, 4264-4265

cpol_mem_info (1042-1056): "held already" over 23 buffers, per_gate a literal sum.  The graph key's arena[] (4489-4495)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('traj', 'rayc', 'poly', 'timed', 'vals', 'mask', 'elev', 'coords', 'wgate', 'qmelt', 'fwmelt',
         'key', 'pos', 'par', 'count', 'totals', 'blkranked', 'rec', 'vmask', 'offset', 'perm', 'res',
         'vn', 'icefirst', 'proj', 'colin', 'xscr', 'xgeo', 'beam', 'bsigma', 'bon',
         'gscan', 'defer', 'present', 'ticket', 'units', 'szinteg', 'clk')
HEAD = ('n_rays', 'ng', 'n_sub', 'n_h', 'n_v', 'n_vars', 'n_hyd', 'n_keys', 'n_vb', 'mode', 'flags', 'cthreads', 'forms', 'g1r', 'tag')
TAIL = ('cnt_stride', 'unit_cap', 'xscr_mask', 'xscr_elev', 'xgeo_lons', 'xgeo_dist', 'xgeo_heights', 'xgeo_elev', 'xgeo_mlmask',
        'key_mask', 'n_col')
MAX_HYDRO, MAX_VARS, MAX_COLS = 8, 24, 30
WIDTH = len(HEAD) + len(NAMES) + len(TAIL)
WIDE = WIDTH + 2 * MAX_COLS
GEO_NP, MAX_PAR, N_SZ, COUNT_SLOTS, HOST_PATHS = 9, 6, 12, 1024, 2
# cpol_mem_info's work[] (1042-1045) and the buffers whose bytes per sub-beam gate its per_gate sums (1052-1056)
HELD = {'traj', 'wgate', 'rayc', 'beam', 'vals', 'mask', 'elev', 'coords', 'qmelt', 'fwmelt', 'key', 'par', 'units', 'perm', 'res',
        'pos', 'vn', 'proj', 'rec', 'vmask', 'gscan', 'defer', 'szinteg'}
PER_GATE = {'vals', 'mask', 'elev', 'qmelt', 'fwmelt', 'vmask', 'proj', 'wgate', 'key', 'pos', 'par', 'rec', 'perm', 'res', 'vn'}
# the work buffers among the 35 entries of the graph key's arena[] (4489-4495; cnt_p and tot_p point into count and totals; the
# other entries are the per-ray tables, the stream and the table set's polynomials); present only with f.gate1_ray
PARENT_KEY = {'traj', 'vals', 'mask', 'elev', 'qmelt', 'fwmelt', 'key', 'pos', 'par', 'count', 'offset', 'units', 'totals', 'perm',
              'res', 'vn', 'icefirst', 'wgate', 'blkranked', 'rec', 'vmask', 'rayc'}


def per_gate_literal(n_vars, n_hyd):
    return n_vars * 4 + 1 + 4 + 8 + 16 + 1 + 8 + 8 + n_hyd * (4 + 4 + MAX_PAR * 8 + 16 + 4 + N_SZ * 8 + 16)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('buffers') / 'buffers_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'c_host', 'buffers_check.cpp'), '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def records(exe, command, width, chunk=65536):
    """The records of a walk, a chunk at a time: {column: int64 array}, the work buffers under their names."""
    proc = subprocess.Popen([exe, command, '-'], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    total = 0
    while True:
        raw = proc.stdout.read(chunk * width * 8)
        if not raw:
            break
        a = np.frombuffer(raw, dtype=np.int64).reshape(-1, width)
        total += len(a)
        r = {name: a[:, i] for i, name in enumerate(HEAD + NAMES + TAIL)}
        if width == WIDE:
            r['col_bytes'] = a[:, WIDTH:WIDTH + MAX_COLS]
            r['col_off'] = a[:, WIDTH + MAX_COLS:]
        yield r
    err = proc.stderr.read().decode()
    assert proc.wait(timeout=60) == 0 and 'BUFFERS_RECORDS %d' % total in err, err


def pad256(x):
    return (x + 255) // 256 * 256


def bit(v, k):
    return (v >> k) & 1


def expected(r):
    """Bytes, the derived values and the offsets as the parent's lines give them; works on int64 columns and on Python integers."""
    n_rays, ng, n_sub, n_h, n_v = r['n_rays'], r['ng'], r['n_sub'], r['n_h'], r['n_v']
    n_vars, n_hyd, n_keys, n_vb = r['n_vars'], r['n_hyd'], r['n_keys'], r['n_vb']
    dbg, ml, dop, dop3, broaden, timed, cols, on_dev, export, present = (bit(r['flags'], k) for k in range(10))
    ray_prep, prep_paths, geo_poly, rvel_terms, gate1, gate1_ray, rare_direct, subsum = (bit(r['forms'], k) for k in range(8))
    n_rg = n_rays * ng
    n_sbg = n_rg * n_sub
    e = {}
    e['traj'] = ((r['mode'] == HOST_PATHS) | dbg | prep_paths) * (n_rays * n_v * 3 * ng * 4)
    e['rayc'] = ray_prep * ((n_rays * n_h + n_rays) * 2 * 8)
    e['poly'] = geo_poly * (n_rays * n_h * 2 * GEO_NP * 8)
    e['timed'] = timed * (2 * n_rays * 4)
    e['vals'] = n_vars * n_sbg * 4
    e['mask'] = n_sbg
    e['elev'] = n_sbg * 4
    e['coords'] = dbg * (n_sbg * 2 * 4)
    e['wgate'] = ml * (n_sbg * 8)
    e['qmelt'] = 2 * n_sbg * 4
    e['fwmelt'] = 2 * n_sbg * 8
    e['key'] = n_hyd * n_sbg * 4
    e['pos'] = n_hyd * n_sbg * 4
    e['par'] = n_hyd * MAX_PAR * n_sbg * 8
    e['cnt_stride'] = n_keys + 3 + COUNT_SLOTS
    e['count'] = 2 * e['cnt_stride'] * 4
    e['totals'] = 2 * 4 * 8 + 0 * n_rays
    e['blkranked'] = (n_sbg + r['cthreads'] - 1) // r['cthreads'] * 4
    e['rec'] = n_hyd * n_sbg * 16
    e['vmask'] = n_sbg
    e['offset'] = 2 * n_keys * 4
    e['perm'] = n_hyd * n_sbg * 4
    e['res'] = n_hyd * n_sbg * N_SZ * 8
    e['vn'] = dop * (n_hyd * n_sbg * 2 * 8)
    e['icefirst'] = dop * (n_rays * n_sub * 24)
    e['proj'] = (dop & rvel_terms) * (n_sbg * 8)
    # columns: the variables, then mask, elev, wgate, q_melt, fw_melt, has_melting where given
    rest = (n_sbg, n_sbg * 4, n_sbg * 8, 2 * n_sbg * 4, 2 * n_sbg * 8, n_rays * n_sub)
    col_bytes = [cols * (n_vars > v) * (n_sbg * 4) for v in range(MAX_VARS)]     # (by position: slot v is a variable while v < n_vars)
    e['rest_bytes'] = [cols * bit(r['flags'], 10 + q) * rest[q] for q in range(6)]
    e['var_bytes'] = col_bytes
    e['colin'] = cols * (1 - on_dev) * (n_vars * pad256(n_sbg * 4) + sum(pad256(b) for b in e['rest_bytes']))
    e['n_col'] = cols * (n_vars + 6)
    xa8, xa4, xa1 = pad256(n_sbg * 8), pad256(n_sbg * 4), pad256(n_sbg)
    e['xscr'] = export * (n_vars * xa4 + xa1 + xa4)
    e['xgeo'] = export * (2 * xa8 + 3 * xa4 + xa1)
    e['xscr_mask'] = export * (n_vars * xa4)
    e['xscr_elev'] = export * (n_vars * xa4 + xa1)
    e['xgeo_lons'] = export * xa8
    e['xgeo_dist'] = export * (2 * xa8)
    e['xgeo_heights'] = export * (2 * xa8 + xa4)
    e['xgeo_elev'] = export * (2 * xa8 + 2 * xa4)
    e['xgeo_mlmask'] = export * (2 * xa8 + 3 * xa4)
    e['beam'] = dop3 * (n_sbg * n_vb * 4)
    e['bsigma'] = (dop3 & broaden) * (n_sbg * 8)
    e['bon'] = (dop3 & broaden) * (n_rays * n_sub * 4)
    e['gscan'] = gate1 * (3 * n_rg * 4)
    e['defer'] = gate1 * n_rg
    e['present'] = (gate1_ray & present) * (n_rays * ((ng + 63) // 64) * 4)
    e['ticket'] = (gate1_ray * (r['g1r'] == 3)) * (n_rays * 4)
    e['unit_cap'] = rare_direct * (n_hyd * n_sbg) + (1 - rare_direct) * (n_hyd * n_sbg // 64 + n_keys + 64)
    e['units'] = (1 - rare_direct) * (e['unit_cap'] * 16)
    e['szinteg'] = (dbg | subsum) * (n_rg * n_hyd * N_SZ * 4)
    e['clk'] = (dbg & (1 - export)) * (2048 * 4 * 8)
    return e


def compare(r, e, seen):
    for name in NAMES + TAIL:
        if name == 'key_mask':
            continue
        bad = np.flatnonzero(np.asarray(r[name] != e[name]))
        assert bad.size == 0, (name, {k: int(r[k][bad[0]]) for k in HEAD}, int(r[name][bad[0]]), int(np.asarray(e[name])[bad[0]]))
        if name in NAMES:
            seen[name] |= {bool(x) for x in np.unique(np.asarray(e[name]) != 0)}


def test_bytes_conditions_and_derived_values_over_the_enumerated_space(exe):
    seen = {name: set() for name in NAMES}
    n = 0
    outside = {}
    for r in records(exe, 'walk', WIDTH):
        e = expected(r)
        compare(r, e, seen)
        n += len(r['n_rays'])
        # the graph key: every buffer a graphable call sizes is in the key's list ...
        graphable = bit(r['forms'], 8) == 1
        for w, name in enumerate(NAMES):
            sized = graphable & (e[name] != 0)
            assert np.all(bit(r['key_mask'], w) == (e[name] != 0)), name          # (graphable or not; and nothing the call did not size)
            # ... and the same calls against the parent's hand list
            listed = (name in PARENT_KEY) | ((name == 'present') & (bit(r['forms'], 5) == 1))
            miss = sized & ~np.asarray(listed)
            if miss.any():
                outside[name] = outside.get(name, 0) + int(miss.sum())
    assert n == 438336
    # every buffer needed by some call and, unless it is needed always, left out by another
    always = {'vals', 'mask', 'elev', 'qmelt', 'fwmelt', 'key', 'pos', 'par', 'count', 'totals', 'blkranked', 'rec', 'vmask', 'offset',
              'perm', 'res'}
    for name in NAMES:
        assert seen[name] == ({True} if name in always else {True, False}), name
    # The finding: graphable calls size six buffers that the parent's list did not hold -- the coordinate polynomials of a sweep
    # with four sub-beams or more, its velocity terms and per-species sums, the scan terms and deferred gates of every
    # single-beam sweep (the default launch sequence of a c2 sweep) and the tickets of CPOL_GATE1_RAY=3.  Each is grow-only on a
    # shape (rays x nodes, gates without the sub-beams) that can grow while every listed buffer stays: a live hazard.
    assert set(outside) == {'poly', 'proj', 'gscan', 'defer', 'ticket', 'szinteg'}, outside


def test_columns_inputs_and_their_staging_offsets(exe):
    seen = {name: set() for name in NAMES}
    n = 0
    for r in records(exe, 'columns', WIDE):
        e = expected(r)
        compare(r, e, seen)
        n += len(r['n_rays'])
        off = 0 * r['n_rays']
        for k in range(MAX_COLS):
            # slot k: variable k while k < n_vars, then the six others in their order, then nothing
            want = e['var_bytes'][k] if k < MAX_VARS else 0 * off
            for q in range(6):
                want = want + (r['n_vars'] + q == k) * e['rest_bytes'][q]
            assert np.array_equal(r['col_bytes'][:, k], want), k
            used = k < r['n_col']
            assert np.array_equal(r['col_off'][:, k][used], off[used]) and np.all(off % 256 == 0), k
            off = off + pad256(want)
        host = bit(r['flags'], 7) == 0
        assert np.array_equal(r['colin'][host], off[host]) and np.all(r['colin'][~host] == 0)
    assert n == 3 * 4 * 4 * 3 * 2 * 64
    assert seen['colin'] == {True, False}


def test_no_32_bit_wrap_at_the_largest_call(exe):
    """2^31 - 1 sub-beam gates, CPOL_MAX_HYDRO species, CPOL_MAX_VARS variables: the planned bytes equal Python's integers."""
    n = 0
    for r in records(exe, 'big', WIDE):
        for i in range(len(r['n_rays'])):
            row = {k: int(r[k][i]) for k in HEAD + NAMES + TAIL}
            assert row['n_rays'] * row['ng'] * row['n_sub'] == 2 ** 31 - 1 and row['n_hyd'] == MAX_HYDRO and row['n_vars'] == MAX_VARS
            e = expected(row)
            for name in NAMES + TAIL:
                if name != 'key_mask':
                    assert row[name] == int(e[name]), (name, row[name], int(e[name]))
            assert row['res'] == 8 * (2 ** 31 - 1) * 96 and row['res'] > 2 ** 40
            if bit(row['flags'], 3):
                assert row['beam'] == (2 ** 31 - 1) * 4097 * 4
            if bit(row['flags'], 6):
                assert int(r['col_off'][i][MAX_COLS - 1]) > 2 ** 37
            n += 1
    assert n == 7 * 2 * 4


def test_table_rows_per_gate_and_held(exe):
    out = subprocess.run([exe, 'table'], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows, per_gate, consts = [], {}, None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == 'row':
            rows.append((NAMES[int(w[1])],) + tuple(int(x) for x in w[2:]))      # (row w of the table is buffer w of the enum)
        elif w[0] == 'per_gate':
            per_gate[(int(w[1]), int(w[2]))] = int(w[3])
        elif w[0] == 'consts':
            consts = tuple(int(x) for x in w[1:])
    assert consts == (len(NAMES), MAX_HYDRO, MAX_VARS, 4, N_SZ, MAX_COLS)
    assert len(rows) == len(NAMES)
    # per_gate equals the parent's literal sum for every (n_hydro, n_vars); the rows that count are the fifteen it restated
    assert len(per_gate) == MAX_HYDRO * MAX_VARS
    for (n_hyd, n_vars), v in per_gate.items():
        assert v == per_gate_literal(n_vars, n_hyd), (n_hyd, n_vars)
    assert {r[0] for r in rows if r[4]} == PER_GATE and len(PER_GATE) == 15
    # "held already" is exactly the parent's 23 buffers
    assert {r[0] for r in rows if r[5]} == HELD and len(HELD) == 23
    # a row's bytes per sub-beam gate are what the parent's line multiplies n_sbg by
    gate = {'vals': (0, 4, 0), 'mask': (1, 0, 0), 'elev': (4, 0, 0), 'coords': (8, 0, 0), 'wgate': (8, 0, 0), 'qmelt': (8, 0, 0),
            'fwmelt': (16, 0, 0), 'key': (0, 0, 4), 'pos': (0, 0, 4), 'par': (0, 0, MAX_PAR * 8), 'rec': (0, 0, 16), 'vmask': (1, 0, 0),
            'perm': (0, 0, 4), 'res': (0, 0, N_SZ * 8), 'vn': (0, 0, 16), 'proj': (8, 0, 0), 'bsigma': (8, 0, 0)}
    for r in rows:
        assert r[1:4] == gate.get(r[0], (0, 0, 0)), r[0]
    # the fills on replacement: the counter sets and the tickets zero, the presence words all ones (3675-3676, 3744, 3750)
    assert {r[0]: r[6] for r in rows if r[6]} == {'count': 1, 'totals': 1, 'ticket': 1, 'present': 2}
