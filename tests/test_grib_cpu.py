"""GRIB edition 1 on the host (cosmo_pol_amd/grib1.py, model_io): the octet layout against a message assembled by hand,
the writer / decoder round trip within the bound the writer's rounding gives, read_model_file on GRIB against the same
decoded fields in an .npz, and what is refused.  No GRIB library and no DWD file exists here: parity with pycosmo's own
numbers stays unpinned (as for the NetCDF path)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import _grib  # noqa: E402
from cosmo_pol_amd import grib1, model_io  # noqa: E402

# One message assembled by hand from the octet tables of WMO FM 92 (not by grib1's writer): centre 78, table 2, parameter
# 11, level type 110, levels 1 / 2, 2014-08-13 12:00, D = 1; rotated grid 3 x 2, La1 -4.400, Lo1 -6.800, La2 -4.390,
# Lo2 -6.780, Di = Dj = 10, scanning 0x40, southern pole -43.000 / 10.000; E = -3, R = 0xC276A000 = -118.625, 12 bits,
# X = 0, 1, 2, 1000, 4095, 7
KNOWN = ('475249420000660100001c024e00ff800b6e01020e080d0c00010000000000001500000100002a00ff0a00030002801130801a9080801126'
         '801a7c000a000a400000000080a7f800271000000000000014008003c276a0000c0000010023e8fff00737373737')
KNOWN_BITS = [0xc13dcccd, 0xc13d999a, 0xc13d6666, 0x3f233333, 0x421d4ccd, 0xc13c6666]


def test_known_answer_message(tmp_path):
    buf = bytes.fromhex(KNOWN)
    assert len(buf) == 102
    (m,) = grib1.scan(buf)
    want = {'length': 102, 'table': 2, 'centre': 78, 'parameter': 11, 'level_type': 110, 'level1': 1, 'level2': 2,
            'year_of_century': 14, 'month': 8, 'day': 13, 'hour': 12, 'minute': 0, 'time_unit': 1, 'P1': 0, 'time_range': 0,
            'century': 21, 'D': 1, 'NV': 0, 'representation': 10, 'Ni': 3, 'Nj': 2, 'La1': -4400, 'Lo1': -6800,
            'La2': -4390, 'Lo2': -6780, 'Di': 10, 'Dj': 10, 'scanning': 0x40, 'pole_lat': -43000, 'pole_lon': 10000,
            'E': -3, 'R': -118.625, 'n_bits': 12, 'unused_bits': 0, 'data_offset': 89, 'n_octets': 9, 'refused': None}
    assert {k: m[k] for k in want} == want
    v = grib1.decode(m, buf)
    assert v.dtype == np.float32 and v.shape == (2, 3)
    assert [int(x) for x in v.view(np.uint32).ravel()] == KNOWN_BITS          # row 0 = the first three
    assert np.array_equal(v, np.array([[-11.8625, -11.85, -11.8375], [0.6375, 39.325, -11.775]], np.float32))
    assert grib1.message_time(m) == '2014-08-13 12:00'
    f = tmp_path / 'one.grb'
    f.write_bytes(b'\x00' * 5 + buf + b'\x00\x00\x00')                        # padding around the message
    g = grib1.Grib1File(str(f))
    try:
        assert g.names() == {'T'} and list(g.fields['T']) == [0]              # T on full level 0
        assert [int(x) for x in g.get('T')[0].view(np.uint32).ravel()] == KNOWN_BITS
        assert g.proj_info() == {'Lo1': -6.8, 'La1': -4.4, 'Lo2': -6.78, 'La2': -4.39,
                                 'Latitude_of_southern_pole': -43.0, 'Longitude_of_southern_pole': 10.0}
    finally:
        g.close()


def test_ibm_singles():
    for bits, val in ((0x41100000, 1.0), (0x42640000, 100.0), (0x3F100000, 2.0 ** -8), (0x00000000, 0.0),
                      (0xC276A000, -118.625)):
        assert grib1.ibm_to_float(bits) == val
        assert grib1.float_to_ibm_down(val) == bits
    for v in (0.1, -0.1, 1e-3, 287.15, -1e-7, 12345.678):
        r = grib1.ibm_to_float(grib1.float_to_ibm_down(v))
        assert r <= v and (v - r) <= abs(v) * 2.0 ** -20                      # rounded DOWN, within the format's precision


def _check_round_trip(path, fields, table):
    g = grib1.Grib1File(path, table)
    try:
        assert g.names() == set(fields)
        for name, orig in fields.items():
            got = g.get(name)
            assert got.dtype == np.float32 and got.shape == orig.shape, name
            for k, m in enumerate(g.planes(name)):
                # |X - (s - R) / 2**E| <= 0.5 (the writer's rint) -> half a step in the scaled value, and one rounding to
                # float32: no measured margin
                bound = 0.5 * 2.0 ** m['E'] / 10.0 ** m['D'] + np.spacing(np.abs(orig[k]))
                err = np.abs(got[k].astype(np.float64) - orig[k].astype(np.float64))
                assert np.all(err <= bound), (name, k, float(err.max()), float(bound.min()))
    finally:
        g.close()


@pytest.mark.parametrize('D', [0, 2, -1])
@pytest.mark.parametrize('n_bits', [8, 12, 16, 24])
@pytest.mark.parametrize('two_mom', [False, True])
def test_round_trip_within_the_writers_rounding(tmp_path, two_mom, n_bits, D):
    raw, hhl, rlon, rlat = _grib.raw_cube(two_mom)
    table = _grib.TABLE_2MOM if two_mom else None
    f, c = _grib.write_pair(tmp_path, raw, hhl, rlon, rlat, n_bits=n_bits, decimal_scale=D, table=table)
    _check_round_trip(f, raw, table)
    _check_round_trip(c, {'HHL': hhl}, table)


def test_round_trip_edge_widths_odd_grid_and_north_to_south(tmp_path):
    rng = np.random.default_rng(11)
    ny, nx = 5, 7                                                           # 35 values x 12 bits: not a multiple of 8
    rlon, rlat = -1.0 + 0.02 * np.arange(nx), 0.5 + 0.02 * np.arange(ny)
    fields = {'T': rng.uniform(200, 300, (3, ny, nx)).astype(np.float32),
              'P': np.full((3, ny, nx), 2.5, np.float32),                    # a constant field
              'U': rng.normal(0, 20, (3, ny, nx)).astype(np.float32)}
    f = str(tmp_path / 'edge.grb')
    grib1.write_grib1(f, fields, rlon, rlat, _grib.SOUTH_POLE, n_bits={'T': 12, 'P': 0, 'U': 32})
    _check_round_trip(f, fields, None)
    g = grib1.Grib1File(f)
    try:
        assert [m['n_bits'] for m in g.planes('P')] == [0, 0, 0] and np.array_equal(g.get('P'), fields['P'])
        assert g.planes('T')[0]['n_octets'] == 53 + 0 and (11 + g.planes('T')[0]['n_octets']) % 2 == 0
        assert g.planes('T')[0]['unused_bits'] == 8 * 53 - 35 * 12
        south_first = g.get('T')
    finally:
        g.close()
    f2 = str(tmp_path / 'north_first.grb')
    grib1.write_grib1(f2, fields, rlon, rlat, _grib.SOUTH_POLE, n_bits={'T': 12, 'P': 0, 'U': 32}, scanning=0x00, pad=3)
    g = grib1.Grib1File(f2)
    try:
        assert g.first['scanning'] == 0x00 and g.first['La1'] == 580 and g.first['La2'] == 500
        assert np.array_equal(g.get('T'), south_first)                       # flipped back: row 0 is the southern one
        assert g.proj_info()['La1'] == 0.5 and g.proj_info()['La2'] == 0.58
    finally:
        g.close()


@pytest.mark.parametrize('two_mom', [False, True])
def test_read_model_file_gives_the_dict_of_the_decoded_fields(tmp_path, two_mom):
    raw, hhl, rlon, rlat = _grib.raw_cube(two_mom, edr=True)
    table = _grib.TABLE_2MOM
    f, c = _grib.write_pair(tmp_path, raw, hhl, rlon, rlat, table=table, time=(2014, 8, 13, 12, 0), step_hours=3)
    m = model_io.read_model_file(f, c, want_refractivity=True, want_edr=True, grib_table=table)
    dec = _grib.decoded(f, table)
    assert set(dec) == set(raw)
    z = str(tmp_path / 'decoded.npz')
    pi = {'Lo1': rlon[0], 'La1': rlat[0], 'Lo2': rlon[-1], 'La2': rlat[-1],
          'Latitude_of_southern_pole': _grib.SOUTH_POLE[0], 'Longitude_of_southern_pole': _grib.SOUTH_POLE[1]}
    model_io.write_npz(z, dec, hhl=_grib.decoded(c, table)['HHL'], proj_info=pi)
    want = model_io.read_model_file(z, want_refractivity=True, want_edr=True)
    assert set(m['data']) == set(want['data']) and 'N' in m['data'] and 'EDR' in m['data']
    for k, v in want['data'].items():
        assert m['data'][k].dtype == np.float32 and np.array_equal(m['data'][k].view(np.uint32), v.view(np.uint32)), k
    assert np.array_equal(m['zlevels'].view(np.uint32), want['zlevels'].view(np.uint32))
    assert m['scheme'] == want['scheme'] == ('2mom' if two_mom else '1mom') and m['derived_from_raw']
    assert set(m['proj_info']) == set(model_io.PROJ_KEYS)
    for k in model_io.PROJ_KEYS:
        assert abs(m['proj_info'][k] - pi[k]) < 1e-12, k
    assert np.allclose(m['resolution'], (0.02, 0.02), rtol=0, atol=1e-12)
    assert m['time'] == '2014-08-13 15:00'
    # without the 2-moment codes the same file is a 1-moment one
    assert model_io.read_model_file(f, c)['scheme'] == '1mom'


def _one_message(**kw):
    rng = np.random.default_rng(5)
    return grib1.encode_message(rng.uniform(250, 300, (4, 6)), 2, 11, 110, (1, 2), -1.0 + 0.02 * np.arange(6),
                                0.5 + 0.02 * np.arange(4), _grib.SOUTH_POLE, **kw)


def _patched(msg, index, value):
    out = bytearray(msg)
    out[index] = value
    return bytes(out)


def test_refusals(tmp_path):
    msg = _one_message()
    assert len(msg) == 8 + 28 + 42 + (11 + 48 + 1) + 4                  # BDS padded to an even length

    def read(data):
        f = tmp_path / 'case.grb'
        f.write_bytes(data)
        return model_io._Grib1(str(f))

    read(msg).close()
    # outside the subset: NotImplementedError naming what was met, pycosmo and the conversion
    cases = {'edition 2': _patched(msg, 7, 2), 'bitmap': _grib.with_bitmap(msg),
             'second-order': _patched(msg, 81, 0x40), 'spherical': _patched(msg, 81, 0x80),
             'integer': _patched(msg, 81, 0x20), 'scanning mode 0x80': _patched(msg, 63, 0x80),
             'scanning mode 0x60': _patched(msg, 63, 0x60), 'representation 50': _patched(msg, 41, 50)}
    for what, data in cases.items():
        with pytest.raises(NotImplementedError, match=what) as e:
            read(data)
        assert 'pycosmo' in str(e.value) and 'cdo -f nc copy' in str(e.value), what
    # a message nobody asks for may be anything (a bitmap on a field the table does not name)
    other = _patched(_grib.with_bitmap(msg), 16, 199)
    src = read(msg + other)
    assert src.names() == {'T'}
    src.close()
    # broken files and inconsistent contents: ValueError
    for what, data in {'truncated': msg[:-20], 'truncated ': msg[:6], '7777': msg[:-4] + b'7778',
                       'two messages': msg + msg}.items():
        with pytest.raises(ValueError, match=what.strip()):
            read(data)
    with pytest.raises(ValueError, match='another grid'):
        read(msg + grib1.encode_message(np.zeros((4, 5)), 2, 33, 110, (1, 2), -1.0 + 0.02 * np.arange(5),
                                        0.5 + 0.02 * np.arange(4), _grib.SOUTH_POLE))
    # a missing level of a needed variable; an accumulation instead of an instantaneous field
    raw, hhl, rlon, rlat = _grib.raw_cube()
    f, c = _grib.write_pair(tmp_path, raw, hhl, rlon, rlat)
    data = open(f, 'rb').read()
    msgs = grib1.scan(data)
    drop = [m for m in msgs if m['parameter'] == 33 and m['table'] == 2 and m['level1'] == 3][0]       # U, level 3
    holed = str(tmp_path / 'holed')
    with open(holed, 'wb') as fh:
        fh.write(data[:drop['offset']] + data[drop['offset'] + drop['length']:])
    with pytest.raises(ValueError, match='U lacks level'):
        model_io.read_model_file(holed, c)
    accum = bytearray(data)
    for m in msgs:
        accum[m['offset'] + 8 + 20] = 4                                      # time-range indicator 4: accumulation
    acc = str(tmp_path / 'accum')
    with open(acc, 'wb') as fh:
        fh.write(bytes(accum))
    with pytest.raises(ValueError, match='time-range indicator 4'):
        model_io.read_model_file(acc, c)
    # a missing variable is the reference's ValueError; the c-file is needed for the heights
    with pytest.raises(ValueError, match='Not all necessary variables'):
        model_io.read_model_file(c, c)
    with pytest.raises(ValueError, match='no level heights'):
        model_io.read_model_file(f)
    # the stub of tests/test_model_io_cpu.py: 'GRIB' + 64 zero octets is edition 0
    stub = str(tmp_path / 'stub.grb')
    with open(stub, 'wb') as fh:
        fh.write(b'GRIB' + b'\x00' * 64)
    with pytest.raises(NotImplementedError, match='pycosmo'):
        model_io.read_model_file(stub)


def test_time_of_forecast_steps():
    base = grib1.scan(_one_message(time=(1999, 12, 31, 23, 30), step_hours=2))[0]
    assert grib1.message_time(base) == '2000-01-01 01:30' and base['century'] == 20 and base['year_of_century'] == 99
    y2k = grib1.scan(_one_message(time=(2000, 2, 28, 12, 0), step_hours=24))[0]
    assert (y2k['century'], y2k['year_of_century']) == (20, 100) and grib1.message_time(y2k) == '2000-02-29 12:00'
    m = dict(base, time_range=10, P1=1, P2=4, time_unit=0)                    # P1 in octets 19-20: 260 minutes
    assert grib1.message_time(m) == '2000-01-01 03:50'


def test_packed_structs_match_the_header(tmp_path):
    """sizeof / offsetof of cpol_packed_plane and cpol_packed_model as gcc sees the header == the ctypes mirrors."""
    from cosmo_pol_amd import _native as N
    pairs = [('cpol_packed_plane', N.PackedPlane), ('cpol_packed_model', N.PackedModel)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cosmo_pol_amd.h"', 'int main(void){']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("consts %d %d %d %d %d %d %d %d\\n", CPOL_MAX_VARS, CPOL_MAX_RAW_FIELDS, CPOL_MAX_LOAD, '
                 'CPOL_RECIPE_COPY, CPOL_RECIPE_HALF_MEAN, CPOL_RECIPE_RHO, CPOL_RECIPE_TIMES_RHO, CPOL_RECIPE_ZEROS);')
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    out = subprocess.check_output([exe]).decode().splitlines()
    got = dict(l.split(None, 1) for l in out)
    for cname, cls in pairs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert [int(x) for x in got['consts'].split()] == [N.MAX_VARS, N.MAX_RAW_FIELDS, N.MAX_LOAD, N.RECIPE_COPY,
                                                       N.RECIPE_HALF_MEAN, N.RECIPE_RHO, N.RECIPE_TIMES_RHO, N.RECIPE_ZEROS]
    for name in ('cpol_stage_model_packed', 'cpol_unpack_planes'):
        assert name in N.EXPORTS and getattr(N.load_library(), name) is not None
