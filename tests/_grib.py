"""Shared by tests/test_grib_cpu.py and tests/test_gpu_grib.py: raw model cubes and the GRIB-1 files written from them."""
import numpy as np

from cosmo_pol_amd import grib1

SOUTH_POLE = (-43.0, 10.0)
# codes of the 2-moment variables and EDR for these tests only (grib1.DEFAULT_TABLE has none): EDR on half levels
TABLE_2MOM = dict(grib1.DEFAULT_TABLE)
TABLE_2MOM.update({(201, 131, 110): 'QH', (201, 132, 110): 'QNH', (201, 133, 110): 'QNR', (201, 134, 110): 'QNS',
                   (201, 135, 110): 'QNG', (201, 136, 110): 'QNI', (201, 152, 109): 'EDR'})


def raw_cube(two_mom=False, shape=(6, 5, 7), seed=3, edr=False, qni=False):
    """In the manner of tests/test_model_io_cpu.py::_raw_cube: -> (raw fields, HHL [nz + 1], rlon, rlat); W (and EDR) on
    half levels."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    hhl = np.linspace(12000., 300., nz + 1)[:, None, None] + rng.uniform(0, 200, (1, ny, nx))
    zf = 0.5 * (hhl[:-1] + hhl[1:])
    T = (288.0 - 6.5e-3 * zf).astype(np.float32)
    P = (101325.0 * np.exp(-zf / 8000.0)).astype(np.float32)
    raw = {'T': T, 'P': P, 'QV': rng.uniform(1e-3, 5e-3, T.shape).astype(np.float32)}
    for k in ('QR', 'QC', 'QI', 'QS', 'QG'):
        raw[k] = rng.uniform(0, 1e-3, T.shape).astype(np.float32)
    for k in ('U', 'V'):
        raw[k] = rng.normal(0, 5, T.shape).astype(np.float32)
    raw['W'] = rng.normal(0, 1, (nz + 1, ny, nx)).astype(np.float32)
    if two_mom:
        raw['QH'] = rng.uniform(0, 1e-4, T.shape).astype(np.float32)
        for k in ('QNH', 'QNR', 'QNS', 'QNG') + (('QNI',) if qni else ()):
            raw[k] = rng.uniform(1, 1e4, T.shape).astype(np.float32)
    if edr:
        raw['EDR'] = (1e-4 + 5e-3 * rng.random((nz + 1, ny, nx))).astype(np.float32)
    rlon = -1.0 + 0.02 * np.arange(nx)
    rlat = 0.5 + 0.02 * np.arange(ny)
    return raw, hhl.astype(np.float32), rlon, rlat


def write_pair(tmp_path, raw, hhl, rlon, rlat, n_bits=16, decimal_scale=0, table=None, stem='lfff00000000', **kw):
    """Model file + c-file (HHL) -> (path, c-path)."""
    f, c = str(tmp_path / stem), str(tmp_path / (stem + 'c'))
    grib1.write_grib1(f, raw, rlon, rlat, SOUTH_POLE, n_bits=n_bits, decimal_scale=decimal_scale, table=table, **kw)
    grib1.write_grib1(c, {'HHL': hhl}, rlon, rlat, SOUTH_POLE, n_bits=n_bits if isinstance(n_bits, int) else 16,
                      table=table, **kw)
    return f, c


def decoded(path, table=None):
    """{name: [n_levels, ny, nx] float32} of every named variable of a file, through the host decoder."""
    g = grib1.Grib1File(path, table)
    try:
        return {k: g.get(k) for k in g.names()}
    finally:
        g.close()


def with_bitmap(msg):
    """A message with a (full) bitmap section put in front of its BDS, lengths mended."""
    msg = bytearray(msg)
    pds_len = int.from_bytes(msg[8:11], 'big')
    gds_len = int.from_bytes(msg[8 + pds_len:11 + pds_len], 'big')
    ni, nj = int.from_bytes(msg[8 + pds_len + 6:8 + pds_len + 8], 'big'), int.from_bytes(msg[8 + pds_len + 8:8 + pds_len + 10], 'big')
    nb = (ni * nj + 7) // 8
    nb += (6 + nb) % 2
    bms = (6 + nb).to_bytes(3, 'big') + bytes([8 * nb - ni * nj, 0, 0]) + b'\xff' * nb
    msg[15] |= 0x40
    cut = 8 + pds_len + gds_len
    out = msg[:cut] + bms + msg[cut:]
    out[4:7] = len(out).to_bytes(3, 'big')
    return bytes(out)
