"""GRIB edition 1 (WMO FM 92): scanner, decoder and writer for the subset COSMO writes -- NumPy only.

What is read: grid-point data in simple packing with floating-point values (BDS flag nibble 0), no bitmap, on a
regular or rotated latitude / longitude grid (GDS representation 0 or 10), 0 ... 32 bits per value, rows scanned
west to east and either south to north (scanning mode 0x40, the model's own order) or north to south (0x00, flipped
on decoding).  Everything else is refused (GribRefused, a NotImplementedError) with a pointer to the ways out.

Octets used (numbered from 1 within their section; multi-octet integers big-endian; latitudes, longitudes, D and E
sign-magnitude with the top bit as the sign):
  IS   1-4 'GRIB', 5-7 total length, 8 edition
  PDS  1-3 length, 4 table version, 8 flag (0x80 GDS present, 0x40 bitmap present), 9 parameter, 10 level type,
       11-12 level(s), 13-17 year of century / month / day / hour / minute, 18 time unit, 19 P1 (20 P2),
       21 time-range indicator, 25 century, 27-28 decimal scale D
  GDS  1-3 length, 4 NV, 5 PV, 6 representation, 7-8 Ni, 9-10 Nj, 11-13 La1, 14-16 Lo1 (millidegrees), 18-20 La2,
       21-23 Lo2, 24-25 Di, 26-27 Dj, 28 scanning mode, 33-35 / 36-38 latitude / longitude of the southern pole
  BDS  1-3 length, 4 flags (high nibble) and unused trailing bits (low nibble), 5-6 binary scale E, 7-10 reference
       value R (IBM hexadecimal single: sign, 7-bit excess-64 power of 16, 24-bit fraction), 11 bits per value,
       12 ... the values, most significant bit first, value i at bit i * n_bits

The decoded value -- the definition the host decoder below and the device kernel (k_grib_unpack) both implement, in
float64: R exactly (every IBM single is a float64), X exactly, t = R + ldexp(X, E) (one rounding), then t / 10**D
for D > 0, t * 10**(-D) for D < 0, nothing for D = 0 (the power of ten built by repeated multiplication by 10.0,
exact up to 10**22), then one rounding to float32.  n_bits = 0 is a constant field: X = 0 in the same statements.

Names: DEFAULT_TABLE maps (table version, parameter, level type) to the variable names of model_io.  The codes are
WMO table 2 and DWD's local table 201 *as remembered*: no DWD or MeteoSwiss file, GRIB library or pycosmo was
available to check them against (nor the level types: COSMO writes W and HHL on half levels, type 109, everything
else here on full levels, type 110).  The 2-moment variables (QH, QNH, QNR, QNS, QNG, QNI) and EDR have no default
entry: a caller who has them passes a table with their codes (`read_model_file(..., grib_table=...)`,
`RadarOperator.grib_table`).  Level type 110 (layer between half levels k and k + 1, octets 11 and 12) is full level
k; type 109 (octets 11-12 as one number) is half level k; level 1 is the model top, the package's level 0.
"""
import datetime
import mmap
import os

import numpy as np

WAY_OUT = ('GRIB input beyond this subset needs pycosmo (cosmo_pol/radar_operator.py:229) or a conversion: write the '
           'file as NetCDF classic (e.g. `fxconvert nc` / `cdo -f nc copy`) or pass arrays to '
           'RadarOperator.load_model_arrays')


class GribRefused(NotImplementedError):
    """A GRIB message outside the accepted subset."""

    def __init__(self, what):
        NotImplementedError.__init__(self, 'GRIB: %s is not read here (edition 1, grid-point data in simple packing, no '
                                           'bitmap, (rotated) lat/lon grid, rows west to east). %s' % (what, WAY_OUT))


# (table version, parameter, level type) -> name: plain data, replaceable (see the module docstring: unverified codes)
DEFAULT_TABLE = {
    (2, 1, 110): 'P', (2, 11, 110): 'T', (2, 33, 110): 'U', (2, 34, 110): 'V', (2, 51, 110): 'QV',
    (2, 40, 109): 'W', (2, 40, 110): 'W', (2, 8, 109): 'HHL',
    (201, 31, 110): 'QC', (201, 33, 110): 'QI', (201, 35, 110): 'QR', (201, 36, 110): 'QS', (201, 39, 110): 'QG',
}

_TIME_UNIT_MINUTES = {0: 1, 1: 60, 2: 1440, 10: 180, 11: 360, 12: 720, 13: 15, 14: 30}


def _u(b, o, n):
    return int.from_bytes(b[o:o + n], 'big')


def _sm(b, o, n):
    """Sign-magnitude integer of n octets."""
    v = _u(b, o, n)
    top = 1 << (8 * n - 1)
    return -(v & (top - 1)) if v & top else v


def ibm_to_float(bits):
    """IBM hexadecimal single (uint32) -> float64, exactly."""
    bits = int(bits)
    frac = bits & 0xFFFFFF
    v = float(np.ldexp(float(frac), 4 * (((bits >> 24) & 0x7F) - 64) - 24))
    return -v if bits >> 31 else v


def float_to_ibm_down(v):
    """The largest IBM hexadecimal single <= v, as uint32 bits."""
    v = float(v)
    if v == 0.0 or not np.isfinite(v):
        if v == 0.0:
            return 0
        raise ValueError('cannot write %r as a GRIB reference value' % (v,))
    a = abs(v)
    _, e2 = np.frexp(a)
    e16 = -((-int(e2)) // 4)                     # ceil(e2 / 4): a / 16**e16 in [1/16, 1)
    frac = float(np.ldexp(a, 24 - 4 * e16))      # exact: a power of two
    f = int(np.floor(frac)) if v > 0 else int(np.ceil(frac))
    if f == 1 << 24:
        f, e16 = 1 << 20, e16 + 1
    char = e16 + 64
    if char > 127:
        raise ValueError('%r is beyond the range of an IBM single' % (v,))
    if char < 0:                                  # below the smallest magnitude
        return 0 if v > 0 else (0x80000000 | 1)
    if f == 0:
        return 0
    return (0x80000000 if v < 0 else 0) | (char << 24) | f


def pow10(n):
    """10.0 ** n for n >= 0 by repeated multiplication (exact up to 10**22; the device does the same)."""
    p = 1.0
    for _ in range(int(n)):
        p *= 10.0
    return p


# ---------------------------------------------------------------------------------------------------- scanner
def scan(buf, name='<buffer>'):
    """Index of the GRIB-1 messages in `buf` (bytes-like): one dict per message with the PDS and GDS fields and, for the
    BDS, `data_offset` (offset of octet 12 in buf), `n_octets`, `n_bits`, `E`, `R`, `unused_bits`.  A message outside
    the accepted subset carries `refused` (what was met) instead of raising: only a message somebody needs is an
    error (GribRefused); a message of another edition cannot be walked at all and is refused here.  Truncated
    messages and a missing 7777 raise ValueError."""
    mv = memoryview(buf)
    n = len(mv)
    out = []
    pos = 0
    find = buf.find if hasattr(buf, 'find') else bytes(mv).find
    while True:
        s = find(b'GRIB', pos)
        if s < 0:
            break
        if s + 8 > n:
            raise ValueError('%s: truncated GRIB message at offset %d' % (name, s))
        head = bytes(mv[s:s + 8])
        total, edition = _u(head, 4, 3), head[7]
        if edition != 1:
            raise GribRefused('edition %d (file %s, offset %d)' % (edition, name, s))
        if s + total > n or total < 8 + 28 + 11 + 4:
            raise ValueError('%s: truncated GRIB message at offset %d (length %d, %d octets left)' % (name, s, total, n - s))
        if bytes(mv[s + total - 4:s + total]) != b'7777':
            raise ValueError('%s: GRIB message at offset %d does not end with 7777' % (name, s))
        out.append(_parse_message(mv, s, total, name))
        pos = s + total
    return out


def _parse_message(mv, s, total, name):
    end = s + total - 4
    p = s + 8
    if p + 28 > end:
        raise ValueError('%s: truncated GRIB message at offset %d (PDS)' % (name, s))
    pds_len = _u(mv, p, 3)
    if pds_len < 28 or p + pds_len > end:
        raise ValueError('%s: GRIB message at offset %d has a PDS of %d octets' % (name, s, pds_len))
    pds = bytes(mv[p:p + 28])
    m = {'offset': s, 'length': total, 'refused': None,
         'table': pds[3], 'centre': pds[4], 'flag': pds[7], 'parameter': pds[8], 'level_type': pds[9],
         'level1': pds[10], 'level2': pds[11], 'level': _u(pds, 10, 2),
         'year_of_century': pds[12], 'month': pds[13], 'day': pds[14], 'hour': pds[15], 'minute': pds[16],
         'time_unit': pds[17], 'P1': pds[18], 'P2': pds[19], 'time_range': pds[20], 'century': pds[24],
         'D': _sm(pds, 26, 2)}
    refuse = []
    p += pds_len
    if m['flag'] & 0x80:
        if p + 32 > end:
            raise ValueError('%s: truncated GRIB message at offset %d (GDS)' % (name, s))
        gds_len = _u(mv, p, 3)
        if gds_len < 32 or p + gds_len > end:
            raise ValueError('%s: GRIB message at offset %d has a GDS of %d octets' % (name, s, gds_len))
        g = bytes(mv[p:p + min(gds_len, 42)])
        m.update({'NV': g[3], 'PV': g[4], 'representation': g[5], 'Ni': _u(g, 6, 2), 'Nj': _u(g, 8, 2),
                  'La1': _sm(g, 10, 3), 'Lo1': _sm(g, 13, 3), 'La2': _sm(g, 17, 3), 'Lo2': _sm(g, 20, 3),
                  'Di': _u(g, 23, 2), 'Dj': _u(g, 25, 2), 'scanning': g[27], 'pole_lat': None, 'pole_lon': None})
        if m['representation'] == 10:
            if gds_len < 42:
                raise ValueError('%s: rotated grid with a GDS of %d octets at offset %d' % (name, gds_len, s))
            m['pole_lat'], m['pole_lon'] = _sm(g, 32, 3), _sm(g, 35, 3)
        if m['representation'] not in (0, 10):
            refuse.append('grid representation %d%s' % (m['representation'],
                                                        ' (spherical harmonics)' if m['representation'] in (50, 60, 70, 80) else ''))
        elif m['scanning'] not in (0x00, 0x40):
            refuse.append('scanning mode 0x%02x' % m['scanning'])
        p += gds_len
    else:
        refuse.append('a message without a grid description section')
    if m['flag'] & 0x40:
        refuse.append('a bitmap section')
        if p + 3 > end:
            raise ValueError('%s: truncated GRIB message at offset %d (BMS)' % (name, s))
        p += _u(mv, p, 3)
    if p + 11 > end:
        raise ValueError('%s: truncated GRIB message at offset %d (BDS)' % (name, s))
    bds_len = _u(mv, p, 3)
    if bds_len < 11 or p + bds_len > end:
        raise ValueError('%s: GRIB message at offset %d has a BDS of %d octets, %d left' % (name, s, bds_len, end - p))
    b = bytes(mv[p:p + 11])
    flags = b[3] >> 4
    if flags & 0x8:
        refuse.append('spherical-harmonic coefficients')
    if flags & 0x4:
        refuse.append('second-order (complex) packing')
    if flags & 0x2:
        refuse.append('integer-valued data')
    if flags & 0x1:
        refuse.append('additional BDS flags (octet 14)')
    m.update({'unused_bits': b[3] & 0xF, 'E': _sm(b, 4, 2), 'R_bits': _u(b, 6, 4), 'R': ibm_to_float(_u(b, 6, 4)),
              'n_bits': b[10], 'data_offset': p + 11, 'n_octets': bds_len - 11})
    if m['n_bits'] > 32:
        refuse.append('%d bits per value' % m['n_bits'])
    if not refuse and m['Ni'] * m['Nj'] * m['n_bits'] > 8 * m['n_octets']:
        raise ValueError('%s: truncated GRIB message at offset %d: %d x %d values of %d bits in %d octets'
                         % (name, s, m['Ni'], m['Nj'], m['n_bits'], m['n_octets']))
    if refuse:
        m['refused'] = ', '.join(refuse)
    return m


def message_time(m):
    """Validity time 'YYYY-MM-DD HH:MM' of an instantaneous field: reference time + P1 time units."""
    tr = m['time_range']
    if tr in (0, 1):
        p1 = m['P1']
    elif tr == 10:
        p1 = (m['P1'] << 8) | m['P2']
    else:
        raise ValueError('GRIB time-range indicator %d (an average, accumulation or difference) is not an '
                         'instantaneous field' % tr)
    if m['time_unit'] not in _TIME_UNIT_MINUTES:
        raise ValueError('GRIB time unit %d is not a fixed span of time' % m['time_unit'])
    ref = datetime.datetime((m['century'] - 1) * 100 + m['year_of_century'], m['month'], m['day'], m['hour'], m['minute'])
    return (ref + datetime.timedelta(minutes=_TIME_UNIT_MINUTES[m['time_unit']] * p1)).strftime('%Y-%m-%d %H:%M')


# ---------------------------------------------------------------------------------------------------- decoder
def unpack_bits(octets, n_values, n_bits):
    """The unsigned integers X [n_values] (uint64) of a simple-packing bit string."""
    if n_bits == 0:
        return np.zeros(n_values, dtype=np.uint64)
    o = np.frombuffer(octets, dtype=np.uint8, count=(n_values * n_bits + 7) // 8)
    if n_bits in (8, 16, 32):
        return o.view({8: 'u1', 16: '>u2', 32: '>u4'}[n_bits])[:n_values].astype(np.uint64)
    if n_bits == 24:
        t = o[:3 * n_values].reshape(n_values, 3).astype(np.uint64)
        return (t[:, 0] << np.uint64(16)) | (t[:, 1] << np.uint64(8)) | t[:, 2]
    bits = np.unpackbits(o)[:n_values * n_bits].reshape(n_values, n_bits)
    full = np.zeros((n_values, 32), dtype=np.uint8)
    full[:, 32 - n_bits:] = bits
    return np.packbits(full, axis=1).view('>u4').reshape(n_values).astype(np.uint64)


def decode_values(octets, n_values, n_bits, R, E, D):
    """float32 [n_values]: the definition of the module docstring."""
    x = unpack_bits(octets, n_values, n_bits).astype(np.float64)
    t = np.float64(R) + np.ldexp(x, int(E))
    if D > 0:
        t = t / pow10(D)
    elif D < 0:
        t = t * pow10(-D)
    with np.errstate(over='ignore'):
        return t.astype(np.float32)


def decode(m, buf):
    """float32 [Nj, Ni] of index entry `m` of `buf`, rows south to north."""
    if m['refused']:
        raise GribRefused(m['refused'])
    ny, nx = m['Nj'], m['Ni']
    v = decode_values(memoryview(buf)[m['data_offset']:m['data_offset'] + m['n_octets']], ny * nx, m['n_bits'],
                      m['R'], m['E'], m['D']).reshape(ny, nx)
    return v[::-1] if m['scanning'] == 0x00 else v


# ---------------------------------------------------------------------------------------------------- a file
class Grib1File(object):
    """The named messages of one file: {name: {0-based level: index entry}} over a read-only mapping of the file.
    Messages the table does not name are skipped; a named one outside the subset raises GribRefused; two messages for
    one (name, level) and named messages on differing grids raise ValueError."""

    def __init__(self, path, table=None):
        self.path = path
        self.table = dict(DEFAULT_TABLE if table is None else table)
        self._f = open(path, 'rb')
        try:
            size = os.fstat(self._f.fileno()).st_size
            self.buf = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ) if size else b''
            self.messages = scan(self.buf, path)
            self.fields = {}
            self.grid = None
            for m in self.messages:
                name = self.table.get((m['table'], m['parameter'], m['level_type']))
                if name is None:
                    continue
                if m['refused']:
                    raise GribRefused('%s (variable %s, file %s, offset %d)' % (m['refused'], name, path, m['offset']))
                lev = (m['level1'] if m['level_type'] == 110 else m['level']) - 1
                if lev < 0:
                    raise ValueError('%s: %s on level 0 (levels count from 1 = model top)' % (path, name))
                m['name'], m['k'] = name, lev
                grid = tuple(m[k] for k in ('representation', 'Ni', 'Nj', 'La1', 'Lo1', 'La2', 'Lo2', 'scanning',
                                            'pole_lat', 'pole_lon'))
                if self.grid is None:
                    self.grid, self.first = grid, m
                elif grid != self.grid:
                    raise ValueError('%s: %s level %d is on another grid than %s' % (path, name, lev + 1, self.first['name']))
                levels = self.fields.setdefault(name, {})
                if lev in levels:
                    raise ValueError('%s: two messages for %s on level %d' % (path, name, lev + 1))
                levels[lev] = m
        except BaseException:
            self.close()
            raise

    def close(self):
        buf, self.buf = getattr(self, 'buf', None), None
        if isinstance(buf, mmap.mmap):
            try:
                buf.close()
            except BufferError:            # (arrays over the mapping are still alive: freed with them)
                pass
        if self._f is not None:
            self._f.close()
            self._f = None

    def names(self):
        return set(self.fields)

    def planes(self, name):
        """Index entries of `name` from level 0 on; ValueError when a level is missing."""
        levels = self.fields[name]
        n = max(levels) + 1
        missing = [k + 1 for k in range(n) if k not in levels]
        if missing:
            raise ValueError('%s: variable %s lacks level(s) %s of %d' % (self.path, name, missing, n))
        return [levels[k] for k in range(n)]

    def n_levels(self, name):
        return len(self.planes(name))

    def get(self, name, levels=None):
        """float32 [n_levels, Nj, Ni] (host decoder); `levels`: only those."""
        pl = self.planes(name)
        if levels is not None:
            pl = [pl[k] for k in levels]
        return np.stack([decode(m, self.buf) for m in pl])

    def shape(self):
        return self.first['Nj'], self.first['Ni']

    def flipped(self):
        return self.first['scanning'] == 0x00

    def proj_info(self):
        m = self.first
        la1, la2 = (m['La2'], m['La1']) if self.flipped() else (m['La1'], m['La2'])
        if m['representation'] == 10:
            pole = (m['pole_lat'] / 1000.0, m['pole_lon'] / 1000.0)
        else:
            pole = (-90.0, 0.0)            # the unrotated grid: the southern pole where it is
        return {'Lo1': m['Lo1'] / 1000.0, 'La1': la1 / 1000.0, 'Lo2': m['Lo2'] / 1000.0, 'La2': la2 / 1000.0,
                'Latitude_of_southern_pole': pole[0], 'Longitude_of_southern_pole': pole[1]}

    def time(self):
        return message_time(self.first)


# ---------------------------------------------------------------------------------------------------- writer
def pack_values(values, n_bits, decimal_scale=0):
    """float array -> (R bits, E, packed octets incl. the pad to an even BDS length, unused bits): R = the (decimally
    scaled) minimum rounded DOWN to an IBM single, E the least exponent with (max - R) <= (2**n_bits - 1) * 2**E,
    X = rint((value - R) / 2**E)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(v)):
        raise ValueError('GRIB simple packing holds finite values only')
    D = int(decimal_scale)
    s = v * pow10(D) if D > 0 else (v / pow10(-D) if D < 0 else v)
    r_bits = float_to_ibm_down(s.min())
    R = ibm_to_float(r_bits)
    rng = float(s.max() - R)
    E = 0
    if n_bits > 0 and rng > 0.0:
        top = float(2 ** n_bits - 1)
        E = int(np.frexp(rng / top)[1])
        while rng <= float(np.ldexp(top, E - 1)):
            E -= 1
        while rng > float(np.ldexp(top, E)):
            E += 1
    if n_bits == 0:
        x = np.zeros(v.size, dtype=np.uint64)
    else:
        x = np.clip(np.rint(np.ldexp(s - R, -E)), 0, float(2 ** n_bits - 1)).astype(np.uint64)
    if n_bits == 0:
        data = b''
    elif n_bits in (8, 16, 32):
        data = x.astype({8: 'u1', 16: '>u2', 32: '>u4'}[n_bits]).tobytes()
    elif n_bits == 24:
        data = np.ascontiguousarray(x.astype('>u4').view(np.uint8).reshape(-1, 4)[:, 1:]).tobytes()
    else:
        bits = np.unpackbits(x.astype('>u4').view(np.uint8).reshape(-1, 4), axis=1)[:, 32 - n_bits:]
        data = np.packbits(bits.reshape(-1)).tobytes()
    pad = (11 + len(data)) % 2
    unused = 8 * (len(data) + pad) - v.size * n_bits
    return r_bits, E, data + b'\x00' * pad, unused


def _sm_bytes(v, n):
    v = int(v)
    return ((abs(v) | (1 << (8 * n - 1))) if v < 0 else v).to_bytes(n, 'big')


def _mdeg(x):
    return int(round(float(x) * 1000.0))


def encode_message(plane, table, parameter, level_type, level, rlon, rlat, south_pole, n_bits=16, decimal_scale=0,
                   time=(2014, 8, 13, 12, 0), step_hours=0, scanning=0x40, centre=78):
    """One GRIB-1 message (bytes) of `plane` [Nj, Ni] (rows south to north): PDS of 28 octets, GDS of 42 (rotated
    lat/lon, NV = 0), BDS padded to an even length.  `level`: k (type 109, half level k, octets 11-12 as one number) or
    (k, k + 1) (type 110).  scanning 0x00 writes the rows north to south."""
    plane = np.asarray(plane)
    ny, nx = plane.shape
    if scanning not in (0x00, 0x40):
        raise ValueError('write_grib1 writes scanning modes 0x40 and 0x00 only')
    rows = plane[::-1] if scanning == 0x00 else plane
    r_bits, E, data, unused = pack_values(rows, n_bits, decimal_scale)
    lev = bytes(level) if isinstance(level, (tuple, list)) else int(level).to_bytes(2, 'big')
    year, month, day, hour, minute = time
    century, yoc = (year - 1) // 100 + 1, (year - 1) % 100 + 1
    pds = ((28).to_bytes(3, 'big') + bytes([table, centre, 255, 255, 0x80, parameter, level_type]) + lev
           + bytes([yoc, month, day, hour, minute, 1, step_hours, 0, 0, 0, 0, 0, century, 0]) + _sm_bytes(decimal_scale, 2))
    la = (rlat[-1], rlat[0]) if scanning == 0x00 else (rlat[0], rlat[-1])
    di = _mdeg((rlon[-1] - rlon[0]) / max(nx - 1, 1))
    dj = _mdeg((rlat[-1] - rlat[0]) / max(ny - 1, 1))
    gds = ((42).to_bytes(3, 'big') + bytes([0, 255, 10]) + nx.to_bytes(2, 'big') + ny.to_bytes(2, 'big')
           + _sm_bytes(_mdeg(la[0]), 3) + _sm_bytes(_mdeg(rlon[0]), 3) + bytes([0x80])
           + _sm_bytes(_mdeg(la[1]), 3) + _sm_bytes(_mdeg(rlon[-1]), 3)
           + min(di, 0xFFFF).to_bytes(2, 'big') + min(dj, 0xFFFF).to_bytes(2, 'big') + bytes([scanning, 0, 0, 0, 0])
           + _sm_bytes(_mdeg(south_pole[0]), 3) + _sm_bytes(_mdeg(south_pole[1]), 3) + bytes(4))
    bds = ((11 + len(data)).to_bytes(3, 'big') + bytes([unused & 0xF]) + _sm_bytes(E, 2) + r_bits.to_bytes(4, 'big')
           + bytes([n_bits]) + data)
    total = 8 + len(pds) + len(gds) + len(bds) + 4
    if total >= 1 << 24:
        raise ValueError('a GRIB-1 message holds less than 16 MiB: %d x %d values of %d bits do not fit' % (ny, nx, n_bits))
    return b'GRIB' + total.to_bytes(3, 'big') + b'\x01' + pds + gds + bds + b'7777'


def write_grib1(path, fields, rlon, rlat, south_pole, n_bits=16, decimal_scale=0, time=(2014, 8, 13, 12, 0),
                step_hours=0, table=None, scanning=0x40, pad=0):
    """Writes {name: [n_levels, Nj, Ni]} as one GRIB-1 file, one message per level, level 0 first.  The codes come from
    `table` ((table version, parameter, level type) -> name; a name with a half-level entry is written on half levels).  `n_bits` / `decimal_scale`: one number, or {name: number}.
    `south_pole` (lat, lon) of the rotated grid; `time` (year, month, day, hour, minute) + `step_hours`; `pad`: octets
    of padding between messages."""
    table = dict(DEFAULT_TABLE if table is None else table)
    codes = {}
    for key, name in table.items():
        if name not in codes or key[2] == 109:          # (a name with both kinds of level is written on half levels)
            codes[name] = key
    per = lambda opt, name: opt.get(name, 16 if opt is n_bits else 0) if isinstance(opt, dict) else opt   # noqa: E731
    with open(path, 'wb') as f:
        for name, cube in fields.items():
            if name not in codes:
                raise ValueError('write_grib1: the table has no code for %s' % name)
            cube = np.asarray(cube)
            tab, par, lt = codes[name]
            for k in range(cube.shape[0]):
                level = (k + 1, k + 2) if lt == 110 else k + 1
                f.write(encode_message(cube[k], tab, par, lt, level, rlon, rlat, south_pole, per(n_bits, name),
                                       per(decimal_scale, name), time, step_hours, scanning))
                f.write(b'\x00' * pad)
