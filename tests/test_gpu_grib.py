"""GRIB-1 model input on the GPU: k_grib_unpack against the host decoder and the device ingest of
RadarOperator.load_model_file (k_grib_unpack + k_model_derive) against model_io.read_model_file + load_model_arrays of
the same files -- bit for bit, on the staged cube as it lies in device memory and through the public interface."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import _grib  # noqa: E402

pytestmark = pytest.mark.gpu

_LUTS = {}


def _luts(hydrometeors, frequency, scheme):
    from cosmo_pol_amd import synthetic
    for h in hydrometeors:
        if (h, frequency, scheme) not in _LUTS:
            _LUTS[(h, frequency, scheme)] = synthetic.make_lut(h, frequency, scheme, n_e=8)
    return {h: _LUTS[(h, frequency, scheme)] for h in hydrometeors}


def _operator(over=None):
    import bench
    from cosmo_pol_amd import RadarOperator
    conf = copy.deepcopy(bench.bench_config(True))
    for sec, kv in (over or {}).items():
        conf.setdefault(sec, {}).update(kv)
    op = RadarOperator(config=conf, luts=_luts, output_variables='only_radar')
    op.grib_table = _grib.TABLE_2MOM
    return op


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _staged(op):
    """(model_v, model_h, model_ht) as they lie in device memory."""
    nz, (ny, nx) = op._zlevels.shape[0], op._zlevels.shape[1:]
    nv = len(op._staged_vars)
    return (op._ctx.debug_read('model_v', (ny, nx, nz, nv), np.float32), op._ctx.debug_read('model_h', (ny, nx, nz), np.float32),
            op._ctx.debug_read('model_ht', (ny, nx, 2), np.float32))


def _host_operator(f, c, over=None, want_n=False, want_edr=False):
    from cosmo_pol_amd import model_io
    op = _operator(over)
    m = model_io.read_model_file(f, c, want_refractivity=want_n, want_edr=want_edr, grib_table=_grib.TABLE_2MOM)
    op.load_model_arrays(m['data'], m['zlevels'], m['proj_info'], m['resolution'], time=m['time'])
    return op


def test_unpack_planes_equal_the_host_decoder_bit_for_bit():
    from cosmo_pol_amd import _native as N, grib1
    ny, nx = 61, 83                                                         # neither a multiple of 64 nor of 8
    n = ny * nx
    rng = np.random.default_rng(20261016)
    ctx = N.Context(0)
    planes, want = [], []
    for n_bits in (0, 1, 7, 12, 16, 24, 31, 32):
        for E in (-12, 0, 5):
            for D in (0, 2, -1):
                for flip in (False, True):
                    x = rng.integers(0, 2 ** n_bits, n, dtype=np.uint64) if n_bits else np.zeros(n, np.uint64)
                    if n_bits:
                        x[[0, n // 2, n - 1]] = 2 ** n_bits - 1               # the largest X of the width, also as the last value
                    if n_bits == 0:
                        octets = np.zeros(0, np.uint8)
                    else:
                        bits = np.unpackbits(x.astype('>u4').view(np.uint8).reshape(-1, 4), axis=1)[:, 32 - n_bits:]
                        octets = np.packbits(bits.reshape(-1))
                    assert octets.size == (n * n_bits + 7) // 8
                    # a buffer that ends on the plane's last octet
                    octets = np.ascontiguousarray(np.concatenate([np.zeros(3, np.uint8), octets])[3:])
                    R = grib1.ibm_to_float(grib1.float_to_ibm_down(float(rng.normal(0, 300))))
                    assert np.array_equal(grib1.unpack_bits(octets, n, n_bits), x)
                    v = grib1.decode_values(octets, n, n_bits, R, E, D).reshape(ny, nx)
                    want.append(v[::-1] if flip else v)
                    planes.append((octets, R, E, D, n_bits, flip, 0, 0))
    got = ctx.unpack_planes(planes, ny, nx)
    ctx.close()
    for i, (p, w) in enumerate(zip(planes, want)):
        assert np.array_equal(_bits(got[i]), _bits(w)), 'plane %d: n_bits %d E %d D %d flip %d' % ((i,) + p[4:5] + p[2:4] + p[5:6])


def test_unpack_planes_refuses_short_buffers():
    from cosmo_pol_amd import _native as N
    ctx = N.Context(0)
    with pytest.raises(ValueError, match='fewer octets'):
        ctx.unpack_planes([(np.zeros(10, np.uint8), 0.0, 0, 0, 16, False, 0, 0)], 4, 4)
    with pytest.raises(ValueError, match='n_bits'):
        ctx.unpack_planes([(np.zeros(100, np.uint8), 0.0, 0, 0, 33, False, 0, 0)], 4, 4)
    ctx.close()


@pytest.mark.parametrize('case', ['1mom', '2mom', '2mom_qni', 'edr', 'north_first', '1mom_nz21', '2mom_nz23'])
def test_device_ingest_stages_the_bits_of_the_host_path(tmp_path, case):
    """A raw cube of 20 x 61 x 83 (W, HHL, EDR on 21 levels) as GRIB + c-file: the staged V, H, HT of load_model_file equal
    those of read_model_file + load_model_arrays on a second operator.  nz = 21 / 23: nz * n_vars is no multiple of 4, so
    k_model_derive stores 4 bytes per lane from rows of odd length, with a last level chunk of 5 / 7 levels."""
    two = case.startswith('2mom')
    nz = int(case[-2:]) if '_nz' in case else 20
    raw, hhl, rlon, rlat = _grib.raw_cube(two, shape=(nz, 61, 83), seed=7, edr=(case == 'edr'), qni=(case == '2mom_qni'))
    rlon, rlat = -1.0 + 0.02 * np.arange(83), -0.3 + 0.02 * np.arange(61)
    kw = {'scanning': 0x00} if case == 'north_first' else {}
    bits = {'T': 16, 'P': 16, 'QV': 16, 'QR': 12, 'QC': 16, 'QI': 24, 'QS': 16, 'QG': 7, 'U': 16, 'V': 16, 'W': 16}
    f, c = _grib.write_pair(tmp_path, raw, hhl, rlon, rlat, n_bits=bits, decimal_scale={'P': -1, 'T': 2},
                            table=_grib.TABLE_2MOM, **kw)
    over = {'doppler': {'scheme': 3, 'turbulence_correction': 1}} if case == 'edr' else None
    op = _operator(over)
    op.load_model_file(f, c)
    assert op._packed is not None                                             # the device path
    assert all(v._data is None for v in op.dic_vars.values())                 # nothing decoded on the host
    ref = _host_operator(f, c, over, want_edr=(case == 'edr'))
    assert ref._packed is None and op._staged_vars == ref._staged_vars
    assert op.config['microphysics']['scheme'] == ('2mom' if two else '1mom')
    assert ('EDR' in op._staged_vars) == (case == 'edr') and len(op._staged_vars) == (15 if two else 9) + (case == 'edr')
    for name, a, b in zip(('model_v', 'model_h', 'model_ht'), _staged(op), _staged(ref)):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), name
    assert op.get_pos_and_time()['time'] == ref.get_pos_and_time()['time'] == '2014-08-13 12:00'
    # the lazily decoded host arrays are the host path's
    for k, v in ref.dic_vars.items():
        assert np.array_equal(_bits(op.dic_vars[k].data), _bits(v.data)), k
    assert np.array_equal(_bits(op.dic_vars['T'].attributes['z-levels']), _bits(ref._zlevels))
    op.close()
    ref.close()


def _sweep_cube():
    """synthetic.small_test_cube's fields turned back into raw model output (mass ratios, pressure, half levels)."""
    from cosmo_pol_amd import model_io, synthetic
    cube = synthetic.small_test_cube(hydrometeors=('R', 'S', 'G'))
    d = {k: v.astype(np.float64) for k, v in cube['data'].items()}
    nz, ny, nx = cube['zlevels'].shape
    raw = {k: d[k].astype(np.float32) for k in ('U', 'V', 'T')}
    for k in ('QR', 'QS', 'QG', 'QI'):
        raw[k] = (d[k + '_v'] / d['RHO']).astype(np.float32)
    raw['QC'] = np.zeros((nz, ny, nx), np.float32)
    raw['QV'] = np.full((nz, ny, nx), 4e-3, np.float32)
    load = sum(raw[k].astype(np.float64) for k in ('QC', 'QR', 'QS', 'QG', 'QI'))
    raw['P'] = (d['RHO'] * model_io.R_D * d['T'] * (1.0 + (model_io.R_V / model_io.R_D - 1.0) * 4e-3 - load)).astype(np.float32)
    w = np.concatenate([d['W'][:1], 0.5 * (d['W'][:-1] + d['W'][1:]), d['W'][-1:]])
    raw['W'] = w.astype(np.float32)
    raw['EDR'] = (1e-4 + 5e-3 * np.random.default_rng(1).random((nz + 1, ny, nx))).astype(np.float32)
    zl = cube['zlevels'].astype(np.float64)
    dz = np.diff(zl, axis=0)
    hhl = np.concatenate([zl[:1] - 0.5 * dz[:1], 0.5 * (zl[:-1] + zl[1:]), zl[-1:] + 0.5 * dz[-1:]])
    pi = cube['proj_info']
    rlon = pi['Lo1'] + cube['resolution'][0] * np.arange(nx)
    rlat = pi['La1'] + cube['resolution'][1] * np.arange(ny)
    return raw, hhl.astype(np.float32), np.round(rlon, 3), np.round(rlat, 3)


def _same(a, b, what):
    assert set(a) == set(b), what
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.shape == b[k].shape and np.array_equal(_bits(v), _bits(b[k])), (what, k)


def test_public_interface_gives_the_same_bits_on_both_paths(tmp_path):
    raw, hhl, rlon, rlat = _sweep_cube()
    f, c = _grib.write_pair(tmp_path, raw, hhl, rlon, rlat, n_bits=16, table=_grib.TABLE_2MOM)
    az, el = np.arange(0.0, 360.0, 30.0), np.full(12, 2.0)
    ref = _host_operator(f, c)
    want = ref.simulate_rays(az, el)
    assert np.isfinite(want['ZH']).sum() > 100                                # the host path alone meets it
    op = _operator()
    op.load_model_file(f, c)
    assert op._packed is not None
    _same(op.simulate_rays(az, el), want, 'simulate_rays')
    a, b = op.get_PPI(2.0, az_step=30.0), ref.get_PPI(2.0, az_step=30.0)
    assert list(a.fields) == list(b.fields) and len(list(a.fields)) >= 10
    for k in a.fields:                                                        # every returned array, the coordinates included
        x, y = a.fields[k]['data'], b.fields[k]['data']
        assert np.array_equal(np.ma.getmaskarray(x), np.ma.getmaskarray(y)), k
        assert np.array_equal(_bits(np.ascontiguousarray(np.ma.getdata(x))), _bits(np.ascontiguousarray(np.ma.getdata(y)))), k
    for k in ('azimuth', 'elevation', 'range', 'fixed_angle'):
        assert np.array_equal(getattr(a, k)['data'], getattr(b, k)['data']), k
    assert a.time['units'] == b.time['units'] == 'seconds since 2014-08-13 12:00'
    op.close()
    ref.close()
    # refraction scheme 2: the refractivity column at the radar comes from the lazily decoded N
    over = {'refraction': {'scheme': 2}}
    ref = _host_operator(f, c, over, want_n=True)
    op = _operator(over)
    op.load_model_file(f, c)
    assert op._packed is not None and op.N._data is None
    got = op.simulate_rays(az, el)
    assert op.N._data is not None
    _same(got, ref.simulate_rays(az, el), 'refraction 2')
    op.close()
    ref.close()


def test_restaging_after_a_configuration_change_and_a_refused_file(tmp_path, capsys):
    raw, hhl, rlon, rlat = _sweep_cube()
    f, c = _grib.write_pair(tmp_path, raw, hhl, rlon, rlat, n_bits=16, table=_grib.TABLE_2MOM)
    az, el = np.arange(0.0, 360.0, 30.0), np.full(12, 2.0)
    d3 = {'doppler': {'scheme': 3, 'turbulence_correction': 0, 'motion_correction': 0}}
    op = _operator(d3)
    op.load_model_file(f, c)
    assert op._packed is not None and 'EDR' not in op._staged_vars
    conf = op.config
    conf['doppler']['turbulence_correction'] = 1
    op.config = conf
    got = op.simulate_rays(az, el)
    assert op._staged_vars[-1] == 'EDR' and op._packed is not None            # staged again, from the index
    fresh = _operator({'doppler': {'scheme': 3, 'turbulence_correction': 1, 'motion_correction': 0}})
    fresh.load_model_file(f, c)
    for name, a, b in zip(('model_v', 'model_h', 'model_ht'), _staged(op), _staged(fresh)):
        assert np.array_equal(_bits(a), _bits(b)), name
    _same(got, fresh.simulate_rays(az, el), 'restaged')
    host = _host_operator(f, c, {'doppler': {'scheme': 3, 'turbulence_correction': 1, 'motion_correction': 0}}, want_edr=True)
    _same(got, host.simulate_rays(az, el), 'restaged vs host path')
    host.close()
    fresh.close()
    # a refused file (bitmap on a needed variable) leaves the operator and its staged cube usable
    from cosmo_pol_amd import grib1
    data = open(f, 'rb').read()
    m = [m for m in grib1.scan(data) if m['parameter'] == 11 and m['table'] == 2][3]
    bad = str(tmp_path / 'bitmap')
    with open(bad, 'wb') as fh:
        fh.write(data[:m['offset']] + _grib.with_bitmap(data[m['offset']:m['offset'] + m['length']]) + data[m['offset'] + m['length']:])
    with pytest.raises(NotImplementedError, match='bitmap'):
        op.load_model_file(bad, c)
    _same(op.simulate_rays(az, el), got, 'after the refusal')
    # a GRIB model file with a non-GRIB c-file takes the host path
    from cosmo_pol_amd import model_io
    cz = str(tmp_path / 'c.npz')
    model_io.write_npz(cz, {}, hhl=_grib.decoded(c)['HHL'])
    op.load_model_file(f, cz)
    assert op._packed is None
    _same(op.simulate_rays(az, el), got, 'npz c-file')
    op.close()
