"""The placement plan of a call's output arrays (cosmo_pol_amd/csrc/cpol_place.h: place_outputs) on the host, through
tests/c_host/place_check.cpp.  No expected value here comes from place_outputs itself: each is stated from the rule as run_sequence
had it before the rule moved (cosmo_pol_hip.hip at commit b5ad419, line numbers of that file):

  the window       pinned mode (outputs_on_device = 2) without debug reads; over every array that is produced and asked for, of
                   the three products alike: lo = the lowest address, hi = the highest end, sum = the bytes of the arrays alone;
                   taken when hi - lo <= sum + sum / 4 + 4096                                         2272-2278, 2704-2714
  the image        skew = lo & 63, extent hi - lo + 64; an array at skew + (its address - lo)         2715-2719, 2724, 2735, 2744
  in place         device mode (1) and asked for; never sz_total while the debug reads are on         2723, 2735, 2744
  own buffers      everything else that is produced: the sweep's arrays each in a buffer of its own whether asked for or not
                   (2725-2726); superobservations and statistics, asked for alone, packed in the order of the list into one
                   block per product, each array padded to 256 bytes                                  1921-1933, 2074-2086
  copies           of arrays in own buffers that are asked for (3509-3512; 1912-1913, 2188-2189); of a `count` array only the
                   rows of requested / folded fields                                                  1914-1916, 2190-2192
                   none in the window form (ONE copy of [lo, hi), 3506-3507) and none of an array written in place (3510)

Which arrays a call produces (2686-2699: no gate coordinates from columns, no float64 mask when mask_sum8 alone is asked for, one
member's geometry) stays with run_sequence; here `produced` is an input, and what the plan does with it is pinned."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP, SUPEROB, STATS = 0, 1, 2
NONE, IN_PLACE, WINDOW, OWN = 0, 1, 2, 3
BASE = 0x7F3A00001000                # a page of the caller's slab


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('place') / 'place_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'c_host', 'place_check.cpp'), '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def A(user, nbytes, produced=1, product=SWEEP, own_under_debug=0, rows=0, mask=0):
    return dict(user=user, bytes=nbytes, produced=produced, product=product, own=own_under_debug, rows=rows, mask=mask)


def plan(exe, mode, debug, arrays):
    args = ['%x:%d:%d:%d:%d:%d:%x' % (a['user'], a['bytes'], a['produced'], a['product'], a['own'], a['rows'], a['mask']) for a in arrays]
    r = subprocess.run([exe, str(mode), str(debug)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {'where': {}, 'copies': [], 'block': {}}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == 'window':
            out.update(window=int(w[1]), lo=int(w[2], 16), hi=int(w[3], 16), skew=int(w[4]), image=int(w[5]))
        elif w[0] == 'block':
            out['block'][int(w[1])] = int(w[2])
        elif w[0] == 'where':
            out['where'][int(w[1])] = (int(w[2]), int(w[3]))
        elif w[0] == 'copy':
            out['copies'].append((int(w[1]), int(w[2]), int(w[3])))
    assert len(out['where']) == len(arrays)
    return out


def pad256(n):
    return (n + 255) // 256 * 256


def disjoint(ranges):
    ranges = sorted(ranges)
    return all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))


def test_window_taken_or_not_at_the_edge(exe):
    sizes = (800, 1600, 800)                                   # multiples of 8: back to back without padding
    total = sum(sizes)
    for gap, taken in ((0, 1), (total // 4 + 4096, 1), (total // 4 + 4097, 0)):
        arrays = [A(BASE, sizes[0]), A(BASE + sizes[0], sizes[1]), A(BASE + sizes[0] + sizes[1] + gap, sizes[2])]
        p = plan(exe, 2, 0, arrays)
        assert p['window'] == taken, gap
        kinds = [p['where'][i][0] for i in range(3)]
        assert kinds == [WINDOW if taken else OWN] * 3
        if taken:
            assert (p['lo'], p['hi']) == (BASE, BASE + total + gap)
        # debug reads on: never; blocking host arrays and device arrays: never
        assert plan(exe, 2, 1, arrays)['window'] == 0
        assert plan(exe, 0, 0, arrays)['window'] == 0
        assert plan(exe, 1, 0, arrays)['window'] == 0
    # only alignment padding between the arrays: 195 float32 values, then a float64 array at the next multiple of 8
    arrays = [A(BASE + 4, 780), A(BASE + 4 + 780, 1560), A(BASE + 2344, 195)]
    assert plan(exe, 2, 0, arrays)['window'] == 1


def test_image_keeps_every_array_aligned_like_its_host_counterpart(exe):
    # the lowest array float32 at a host address 4 mod 8, a float64 array behind it at an 8-aligned address
    lo = BASE + 4
    arrays = [A(lo, 780), A(lo + 780, 1560), A(lo + 780 + 1560, 780, product=SUPEROB), A(lo + 780 + 1560 + 784, 1560, product=STATS)]
    assert lo % 8 == 4 and arrays[1]['user'] % 8 == 0 and arrays[3]['user'] % 8 == 0
    p = plan(exe, 2, 0, arrays)
    assert p['window'] == 1
    hi = arrays[3]['user'] + 1560
    assert (p['lo'], p['hi']) == (lo, hi)
    assert p['skew'] == lo % 64
    consts = set()
    for i, a in enumerate(arrays):
        kind, off = p['where'][i]
        assert kind == WINDOW and off == a['user'] - lo
        consts.add(off + p['skew'] - a['user'])                # image offset + skew - host address
        assert off + p['skew'] + a['bytes'] <= p['image']      # inside the image
    assert len(consts) == 1 and consts.pop() % 64 == 0          # relative to a 64-aligned image base
    assert p['image'] <= hi - lo + 64
    assert p['copies'] == []


def test_no_two_placed_arrays_overlap(exe):
    # one slab, the arrays of the three products interleaved, in an order different from the list's
    sizes = [780, 1560, 2200, 780, 40 * 20, 1560, 780, 4000]
    products = [SWEEP, STATS, SUPEROB, SWEEP, SUPEROB, STATS, SWEEP, STATS]
    order = [5, 2, 7, 0, 3, 6, 1, 4]                          # position in the slab of array i
    addr, at = {}, BASE + 4
    for pos in range(len(sizes)):
        i = order.index(pos)
        addr[i] = at
        at += (sizes[i] + 7) // 8 * 8 - (4 if pos == 0 else 0)
    arrays = [A(addr[i], sizes[i], product=products[i]) for i in range(len(sizes))]
    assert disjoint([(a['user'], a['user'] + a['bytes']) for a in arrays])
    p = plan(exe, 2, 0, arrays)
    assert p['window'] == 1
    assert [p['where'][i] for i in range(len(arrays))] == [(WINDOW, a['user'] - min(addr.values())) for a in arrays]
    assert disjoint([(p['where'][i][1], p['where'][i][1] + a['bytes']) for i, a in enumerate(arrays)])
    assert p['block'] == {SWEEP: 0, SUPEROB: 0, STATS: 0}
    # the same arrays as blocking host arrays: the sweep's each at offset 0 of its own buffer, the others packed per product in
    # the order of the list, at multiples of 256; the block is the padded sum
    p = plan(exe, 0, 0, arrays)
    for product in (SUPEROB, STATS):
        mine = [i for i in range(len(arrays)) if products[i] == product]
        want, off = [], 0
        for i in mine:
            want.append((OWN, off))
            off += pad256(sizes[i])
        assert [p['where'][i] for i in mine] == want
        assert all(p['where'][i][1] % 256 == 0 for i in mine)
        assert p['block'][product] == sum(pad256(sizes[i]) for i in mine)
        assert disjoint([(p['where'][i][1], p['where'][i][1] + sizes[i]) for i in mine])
        assert p['where'][mine[-1]][1] + sizes[mine[-1]] <= p['block'][product]
    assert all(p['where'][i] == (OWN, 0) for i in range(len(arrays)) if products[i] == SWEEP) and p['block'][SWEEP] == 0
    # device arrays: each through the caller's pointer
    p = plan(exe, 1, 0, arrays)
    assert all(p['where'][i] == (IN_PLACE, 0) for i in range(len(arrays))) and p['copies'] == [] and sum(p['block'].values()) == 0


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_one_difference_at_a_time(exe, mode):
    base = [A(BASE, 800), A(BASE + 800, 1600), A(BASE + 2400, 800, product=SUPEROB), A(BASE + 3200, 1024, product=SUPEROB)]
    home = {0: OWN, 1: IN_PLACE, 2: WINDOW}[mode]
    p = plan(exe, mode, 0, base)
    assert [p['where'][i][0] for i in range(4)] == [home] * 4
    # a NULL pointer: a sweep array is still written, into its own buffer, and copied nowhere; another product's array is not
    # written and takes no room in the block; neither widens the window
    for i in (0, 2):
        arrays = [dict(a) for a in base]
        arrays[i]['user'] = 0
        p = plan(exe, mode, 0, arrays)
        assert p['where'][i] == ((OWN, 0) if i == 0 else (NONE, 0))
        assert [p['where'][k][0] for k in range(4) if k != i] == [home] * 3
        assert all(c[0] != i for c in p['copies'])
        if mode == 2:
            assert p['lo'] == (BASE + 800 if i == 0 else BASE)
        if mode == 0 and i == 2:
            assert p['block'][SUPEROB] == 1024 and p['where'][3] == (OWN, 0)
    # not produced: not written whatever the pointer, of either product, and no part of the window
    for i in (0, 2):
        arrays = [dict(a) for a in base]
        arrays[i]['produced'] = 0
        arrays[i]['user'] = BASE + (1 << 30)                    # (far away: it would break the window if it counted)
        p = plan(exe, mode, 0, arrays)
        assert p['where'][i] == (NONE, 0) and all(c[0] != i for c in p['copies'])
        assert [p['where'][k][0] for k in range(4) if k != i] == [home] * 3
    # `mask` when mask_sum8 alone is asked for (run_sequence: not produced, no pointer): no buffer, no copy
    arrays = [dict(a) for a in base] + [A(0, 1600, produced=0)]
    assert plan(exe, mode, 0, arrays)['where'][4] == (NONE, 0)
    # sz_total while the debug reads are on is never written in place: its own buffer, and a copy to the caller's
    arrays = [dict(a) for a in base]
    arrays[1]['own'] = 1
    assert plan(exe, mode, 0, arrays)['where'][1][0] == home
    p = plan(exe, mode, 1, arrays)
    assert p['window'] == 0
    assert p['where'][1] == (OWN, 0) and (1, 0, 1600) in p['copies']
    assert [p['where'][k][0] for k in (0, 2, 3)] == [IN_PLACE if mode == 1 else OWN] * 3


def test_copy_out_list(exe):
    rows, cells = 10, 40
    count = rows * cells * 2
    asked = 0b0000001001                                       # fields 0 and 3
    arrays = [A(BASE, 800), A(0, 800), A(BASE + 800, 1600),
              A(BASE + 2400, 160, product=SUPEROB), A(0, 160, product=SUPEROB), A(BASE + 2560, 160, product=SUPEROB),
              A(BASE + 2720, count, product=SUPEROB, rows=rows, mask=asked)]
    for mode in (1, 2):                                        # in place; the window (ONE copy of [lo, hi), not in the list)
        p = plan(exe, mode, 0, arrays)
        assert p['copies'] == [] and (mode == 1 or p['window'] == 1)
    p = plan(exe, 0, 0, arrays)
    row = cells * 2
    assert sorted(p['copies']) == sorted([(0, 0, 800), (2, 0, 1600), (3, 0, 160), (5, 0, 160), (6, 0 * row, row), (6, 3 * row, row)])
    assert p['where'][6] == (OWN, 2 * 256) and p['block'][SUPEROB] == 2 * 256 + pad256(count)
    # pinned arrays too far apart for a window: the same copies
    far = [dict(a) for a in arrays]
    far[2]['user'] = BASE + (1 << 24)
    q = plan(exe, 2, 0, far)
    assert q['window'] == 0 and sorted(q['copies']) == sorted(p['copies'])
    # the statistics' count: the rows of folded fields alone
    arrays = [A(BASE, 160, product=STATS), A(BASE + 160, count, product=STATS, rows=rows, mask=0b1000000010)]
    p = plan(exe, 0, 0, arrays)
    assert sorted(p['copies']) == [(0, 0, 160), (1, 1 * row, row), (1, 9 * row, row)]
