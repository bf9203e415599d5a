"""RadarOperator: the reference's user-facing API over the HIP hot path.

Same constructor, properties and scan methods as cosmo_pol/radar_operator.py:46
(`RadarOperator(options_file, output_variables)`, `.config` getter/setter,
`set_lut`, `load_model_file`, `get_PPI`, `get_RHI`, `get_VPROF`,
`get_GPM_swath`, `get_pos_and_time`, `close`).  The body of the reference's scan
loop (one `pool.map` task per radial, radar_operator.py:407-432) is replaced by
ONE call into libcosmo_pol_hip.so per sweep; there is no CPU path.

Keyword-only extras: `device`, `lut_dir`, `luts` (pre-built tables {h: table} or a
callable (hydrometeors, frequency, scheme) -> {h: table}),
`load_model_arrays(...)` (pycosmo / GRIB are not available here).
"""
import copy
import datetime
from collections.abc import MutableMapping
import ctypes as C
import os
import threading

import numpy as np

from . import _native as N
from . import config as cfg
from . import constants as K
from . import geometry as geo
from . import hydrometeors as hyd
from . import quadrature
from . import ensemble_stats as ES
from . import ensemble_verify as EV
from . import spectrum_moments as SM
from . import superob as SO
from . import histogram as HG
from . import species as SP
from . import composite as CP
from . import neighbourhood as NB
from . import objects as OB
from .lut import load_all_lut

RADAR_FIELDS = ['ZH', 'ZDR', 'ZV', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V']
DOPPLER_FIELDS = ['RVEL', 'DSPECTRUM']
_DB_FIELDS = ('ZDR', 'ZV', 'ZH')
# entries of device_outputs that are dicts of a product (`product.name`), and what such an entry lacks without its product
_PRODUCT_OUTPUTS = {'histogram': 'a histogram', 'composite': 'a composite', 'stats': 'ensemble statistics', 'moments': 'moments=',
                    'superob': 'superob='}
_COORDS = ('lats', 'lons', 'dist', 'heights')
_ONCE = _COORDS + ('visibility',)             # per geometry row: once, whatever the number of members


class ModelVar(object):
    """Duck type of a pycosmo variable (what interpolation.py:547-561 reads)."""

    def __init__(self, name, data, attributes):
        self.name = name
        self.data = data
        self.attributes = attributes


class LazyModelVar(ModelVar):
    """A ModelVar whose `data` is built on first access (a model ingested on the device keeps the file's index, not
    decoded arrays: the host decoder runs only for a caller who reads them)."""

    def __init__(self, name, make, attributes):
        self.name = name
        self._make = make
        self._data = None
        self.attributes = attributes

    @property
    def data(self):
        if self._data is None:
            self._data = self._make()
        return self._data

    @data.setter
    def data(self, value):
        self._data = value


class LazyDict(MutableMapping):
    """A mapping whose values are built on first access (`add(key, make)`): the containers returned by
    get_PPI / get_RHI / get_GPM_swath carry a dozen derived arrays per scan (dB fields, NaN masks,
    re-gridded beams) of which a caller typically touches a few; building them eagerly -- as the
    reference's PyartRadop / SimulatedGPM do on the host -- cost 4 - 7 x the simulation itself.
    Iteration order = insertion order; every read access goes through the builders.  A full
    MutableMapping (pop, update, setdefault, ==, copy ... see every key; round-3 advisor finding: the
    dict subclass this used to be overrode only part of the dict API); `copy()`, pickling and
    deepcopy build the pending values and give a plain dict."""

    def __init__(self):
        self._make = {}
        self._data = {}             # key -> value, or the sentinel while pending (keeps the insertion order)
        self._build = threading.Lock()      # two threads reading one pending key: built once, by the first

    _PENDING = object()

    def add(self, key, make):
        self._make[key] = make
        self._data[key] = LazyDict._PENDING

    def __getitem__(self, key):
        v = self._data[key]
        if v is LazyDict._PENDING:
            with self._build:
                v = self._data[key]
                if v is LazyDict._PENDING:
                    v = self._data[key] = self._make.pop(key)()
        return v

    def __setitem__(self, key, value):
        self._make.pop(key, None)
        self._data[key] = value

    def __delitem__(self, key):
        del self._data[key]
        self._make.pop(key, None)

    def __iter__(self):
        return iter(list(self._data))

    def __len__(self):
        return len(self._data)

    def __contains__(self, key):
        return key in self._data

    def keys(self):
        return list(self._data)

    def values(self):
        return [self[k] for k in list(self._data)]

    def items(self):
        return [(k, self[k]) for k in list(self._data)]

    def pending(self, key):
        return self._data.get(key) is LazyDict._PENDING

    def copy(self):
        return dict(self.items())

    def __reduce__(self):
        return (dict, (self.copy(),))

    def __deepcopy__(self, memo):
        return copy.deepcopy(self.copy(), memo)

    def __repr__(self):
        return 'LazyDict(%s)' % ', '.join('%r%s' % (k, ' (pending)' if self.pending(k) else '') for k in self._data)


class RadarScan(object):
    """Light stand-in for PyartRadop (cosmo_pol/radar/pyart_wrapper.py:186-342):
    same field names and conventions (ZH, ZV, ZDR in dB with 0 -> NaN, masked
    where NaN, extra 'Latitude', 'Longitude', 'rangearray' fields, one entry of
    sweep_start/stop_ray_index per sweep).  `fields` is a LazyDict: the dB conversion, the
    stacking over the sweeps and the NaN mask of a field are made when the field is first read."""

    def __init__(self, scan_type, elevations, azimuths, ranges, pos_time, sweeps):
        self.scan_type = scan_type
        self.nsweeps = len(sweeps)
        self.range = {'data': np.asarray(ranges)}
        self.latitude = {'data': np.array(pos_time['latitude'], dtype=float)}
        self.longitude = {'data': np.array(pos_time['longitude'], dtype=float)}
        self.altitude = {'data': np.array(pos_time['altitude'], dtype=float)}
        self.time = {'data': np.zeros(len(sweeps[0]['azimuth'])),
                     'units': 'seconds since ' + str(pos_time.get('time'))}
        self.raw = sweeps                       # linear-unit arrays per sweep
        counts = np.array([len(s['azimuth']) for s in sweeps], dtype=np.int64)
        stop = np.cumsum(counts)
        self.azimuth = {'data': np.concatenate([np.asarray(s['azimuth'], dtype=float) for s in sweeps])}
        self.elevation = {'data': np.concatenate([np.asarray(s['elevation'], dtype=float) for s in sweeps])}
        self.sweep_start_ray_index = {'data': (stop - counts).astype(float)}
        self.sweep_stop_ray_index = {'data': (stop - 1).astype(float)}
        self.sweep_number = {'data': np.arange(0, self.nsweeps, dtype=float)}
        self.sweep_mode = {'data': [scan_type] * self.nsweeps}
        self.fixed_angle = {'data': np.array(elevations if scan_type == 'ppi' else azimuths,
                                             dtype=float)}
        self.fields = LazyDict()

        def field(k):
            def make():
                parts = [s['fields'][k] for s in sweeps]
                stack = np.concatenate(parts, axis=0) if (len(parts) > 1 or k in _DB_FIELDS) else parts[0]
                if k in _DB_FIELDS:
                    # dB, 0 -> NaN (pyart_wrapper.py:256-258); in place on the stacked copy
                    with np.errstate(divide='ignore', invalid='ignore'):
                        stack[stack == 0] = np.nan
                        np.log10(stack, out=stack)
                        stack *= 10
                return {'data': np.ma.array(stack, mask=np.isnan(stack), copy=False)}
            return make

        def coords(src):
            def make():
                stack = np.concatenate([s[src] for s in sweeps], axis=0)
                return {'data': np.ma.array(stack, mask=np.isnan(stack)), 'units': ['degrees']}
            return make
        for k in sweeps[0]['fields'].keys():
            self.fields.add(k, field(k))
        self.fields.add('Latitude', coords('lats'))
        self.fields.add('Longitude', coords('lons'))
        self.nrays = len(self.azimuth['data'])
        self.ngates = len(self.range['data'])
        # (the builders capture locals, never `self`: a scan must not be part of a reference cycle, or the
        # page-locked block of its arrays would wait for the cyclic garbage collector instead of
        # returning to the operator's pool when the scan is dropped)
        rng, shape = self.range['data'], (self.nrays, self.ngates)
        self.fields.add('rangearray', lambda: {'data': np.broadcast_to(rng, shape)})

    def to_pyart(self, varray=None):
        """The scan as the reference's PyartRadop (a pyart.core.Radar); needs Py-ART."""
        from .pyart_wrapper import as_pyart_radar
        return as_pyart_radar(self, varray)

    def to_radials(self):
        """The scan as the reference's list of sweeps of Radial records
        (what cut_at_sensitivity / PyartRadop consume, radar_operator.py:445-451): linear
        units, row views of the per-sweep arrays."""
        from .radial import to_radials
        return [to_radials(s) for s in self.raw]

    def get_field(self, sweep_idx, variable):
        i0 = int(self.sweep_start_ray_index['data'][sweep_idx])
        i1 = int(self.sweep_stop_ray_index['data'][sweep_idx]) + 1
        return self.fields[variable]['data'][i0:i1]


def _is_torch(a):
    return type(a).__module__.startswith('torch')


def _host(a):
    return a.cpu().numpy() if _is_torch(a) else np.asarray(a)


def _mask_from_sum(sum8, n_sub):
    """Builder of the radial mask from cpol_outputs.mask_sum8: the two statements of doppler_scatter.py:472-477 on the
    sum of the sub-beams' mask codes (the sum itself comes from the device)."""
    def make():
        if n_sub == 1:
            return sum8.astype(np.float64)          # (one sub-beam: the codes themselves; the (-1, 0] -> 0 rule changes no integer)
        # the two statements on the 256 possible sums, then one gather (5 x faster than the statements on the whole array)
        lut = np.arange(-128, 128) / float(n_sub)
        lut[np.logical_and(lut > -1, lut <= 0)] = 0
        return np.take(lut, sum8.astype(np.intp) + 128)
    return make


_table_serial = [0]


def _table_identity():
    """64-bit identity (never 0) of one staged hydrometeor slot for the library's table caches
    (cpol_hydro_desc.table_id): a process-wide serial stored with the operator's cache entry of the table
    set -- never derived from a memory address, which a later array of other content could re-use."""
    _table_serial[0] += 1
    return (os.getpid() << 32) | _table_serial[0]


class RadarOperator(object):
    _table_serial = 0          # tags of per-ray table sets handed to the library
    _plane_serial = 0          # tags of the per-gate plane coordinates of composites (cpol_composite.plane_version)

    def __init__(self, options_file=None, output_variables='all', *, device=0, lut_dir=None,
                 luts=None, config=None, distributed=False, gather_to=None, lanes=2, backend='hip',
                 pyart_output=False, stencil_budget=None):
        if backend != 'hip':
            # by design: the product path is the HIP library or nothing (no CPU fallback)
            raise N.NativeError("backend %r: only 'hip' exists; the CPU restatement lives under "
                                "oracle/ as test infrastructure and is never used by the product"
                                % (backend,))
        print('Reading options defined in options file')
        self._ctx = N.Context(device)         # raises if the HIP library / GPU is missing
        if stencil_budget is not None:
            # bytes of device memory for gate stencils -- what a single-beam sweep knows of its gates before it reads the model's
            # values, kept per (scan geometry, level heights) from the second time a geometry is seen (69 B per gate); 0: off,
            # None: the library's default (1 GiB)
            self._ctx.set_stencil_budget(stencil_budget)
        self._affinity_before = None
        if distributed:
            # one process per GPU: run this rank's threads next to its GPU (CPOL_NUMA_BIND=0: leave the
            # affinity alone; close() restores what the thread had before); the reference's worker pool is
            # not placed at all (radar_operator.py:402)
            before = os.sched_getaffinity(0) if hasattr(os, 'sched_getaffinity') else None
            self.numa = N.bind_to_device_numa_node(device)
            if self.numa.get('bound'):
                self._affinity_before = before
        self._pool = N.PinnedPool(device)     # page-locked blocks of the results handed to the user
        # lanes: contexts forked from _ctx (shared cube / tables, own stream + work buffers);
        # the sweeps of a volume scan are spread over them so that they overlap on the GPU
        self.lanes = max(1, int(lanes))
        self._lane_ctx = []
        self._lock = threading.RLock()
        self.device = device
        self.distributed = bool(distributed)   # shard the rays of every sweep over the ranks
        self.gather_to = gather_to             # distributed scans: None = every rank gets the scan (all-gather);
                                               # r = rank r alone does (gather; get_PPI returns None elsewhere)
        self._runner = None
        self.pyart_output = bool(pyart_output) # get_PPI / get_RHI return a pyart.core.Radar (needs Py-ART)
        self.reuse_device_tables = True        # keep per-ray tables in HBM between equal sweeps
        self.volume_in_one_sequence = True     # get_PPI / get_RHI: all sweeps of a scan in one launch sequence
        self.pipeline_single_beam_scans = True # ... unless the scan has ONE sub-beam per ray and the operator lanes: a sweep per lane, page-locked outputs, one wait
                                               # (False: sweep by sweep, spread over the lanes)
        self.sequence_memory_budget = None     # bytes of device work buffers ONE launch sequence may need (about 1.2 KB per
                                               # sub-beam gate with six species): a scan beyond it is run as several
                                               # sequences of whole sweeps.  None: a third of the memory free at the time
        self.debug_flags = 0                   # cpol_sweep_params.debug_flags (tests / tools only: N.DEBUG_EXACT_SUBBEAMS)
        self.compact_mask = False              # True: in pinned (non-blocking) host outputs the radial mask crosses PCIe as one byte
                                               # per gate (the sum of the sub-beams' codes, cpol_outputs.mask_sum8) and becomes the
                                               # reference's float64 array -- sum / n_sub, (-1, 0] -> 0: doppler_scatter.py:472-477 --
                                               # on the host when `mask` is first read (0.13 ms per 180 k gates, on the reader's
                                               # thread: worth it for a consumer that seldom reads the mask; measured by bench.py).
                                               # False (the default, and every blocking call): the float64 array from the device
        self.lut_dir = lut_dir
        if lut_dir:
            from . import tablecache
            tablecache.set_default_dir(os.path.join(lut_dir, '.cpol_cache'))   # slow host-side staging tables
        self._user_luts = luts
        self.current_microphys_scheme = '1mom'
        self.dic_vars = None
        self.N = 0
        self.grib_table = None                 # {(table version, parameter, level type): name} replacing grib1.DEFAULT_TABLE
        self._packed = None                    # a model ingested on the device: the open GRIB sources (load_model_file)
        self._zl = None
        self.lut_sz = None
        self._model_staged = False
        self._staged_serial = 0
        self._n_members = 0                    # ensemble members staged beside the model (load_model_ensemble); the model is member 0
        self._member = 0                       # the member every ordinary call reads (select_member)
        self.ensemble_shared_from = 4          # form=None of the ensemble calls: 'shared' from this many sub-beams per radial
                                               # (CPOL_RAY_PREP_MIN_SUB: where the sweep's geometry is heavy enough to be worth sharing;
                                               # below it 'per_member' keeps the fused single-beam kernels -- DESIGN.md section 7c)
        self._staged_hydro = None
        self.constants = None
        if output_variables in ['all', 'only_model', 'only_radar']:
            self.output_variables = output_variables
        else:
            self.output_variables = 'all'
            print("Invalid output_variables input, must be either 'all', 'only_model' or "
                  "'only_radar'")
        conf = config if config is not None else cfg.init(options_file)
        self.config = conf

    # ------------------------------------------------------------------ config
    @property
    def config(self):
        return copy.deepcopy(self.__config)

    @config.setter
    def config(self, config_dic):
        """Validates, derives constants and (re)loads the lookup tables when the
        frequency or the melting switch changed (radar_operator.py:106-159)."""
        if config_dic is None:
            self.__config = None
            return
        print('Loading new configuration...')
        checked = cfg.sanity_check(config_dic)
        old = getattr(self, '_RadarOperator__config', None)
        reload_lut = (old is None or not self.lut_sz
                      or checked['radar']['frequency'] != old['radar']['frequency']
                      or checked['microphysics']['with_melting'] != old['microphysics']['with_melting']
                      or checked['microphysics']['with_ice_crystals'] != old['microphysics']['with_ice_crystals']
                      or checked['microphysics']['scheme'] != old['microphysics']['scheme']
                      or (checked['doppler']['scheme'] == 2) != (old['doppler']['scheme'] == 2)
                      or (checked['doppler']['scheme'] == 3) != (old['doppler']['scheme'] == 3))
        self.__config = checked
        self.constants = K.DerivedConstants(checked)
        self._cache = {}                       # per-configuration host-side tables
        if reload_lut:
            if old is not None:
                print('Reloading lookup tables...')
            self.set_lut()

    def _drop_lanes(self):
        """Closes the forked contexts (before re-staging).  Each is drained first, so that queued
        sweeps complete into their result arrays (which live in the operator's pinned pool, not in
        the lane) and a deferred domain error of a dropped lane is raised, not lost."""
        lanes, self._lane_ctx = self._lane_ctx, []
        err = None
        for c in lanes:
            try:
                c.synchronize()
            except IndexError as e:
                err = e
            c.close()
        if err is not None:
            raise err

    def _lane(self, i):
        """Context of lane i (0 = the root context); lanes are forked on first use and
        dropped whenever the staged model / tables change."""
        if i == 0:
            return self._ctx
        with self._lock:
            while len(self._lane_ctx) < i:
                self._lane_ctx.append(self._ctx.fork())
            return self._lane_ctx[i - 1]

    def close(self):
        if self._ctx is not None:
            try:
                self._drop_lanes()
            except IndexError as e:           # a queued sweep left the model domain and nobody waited for it
                print('RadarOperator.close: %s' % e)
            if self._runner is not None:
                self._runner.drain()
                self._runner = None
            for _, r in self.__dict__.pop('_group_runners', {}).values():
                r.drain()
            self._ctx.close()
            self._ctx = None
            self._pool.close()                # (blocks of results still held are freed with their last view)
            if self._affinity_before is not None:
                try:
                    os.sched_setaffinity(0, self._affinity_before)
                except OSError:
                    pass
                self._affinity_before = None
        self._drop_packed()
        self.dic_vars = None
        self.lut_sz = None
        self.__config = None

    # ------------------------------------------------------------------ tables
    def set_lut(self):
        """Loads the scattering tables of the current configuration and stages
        them (with the per-bin PSD factors) in HBM (radar_operator.py:161-182)."""
        conf = self.__config
        scheme = conf['microphysics']['scheme']
        self.current_microphys_scheme = scheme
        hl = hyd.hydrometeor_list(conf)
        # (Doppler scheme 3 with the melting scheme, round 6: the fall speed of a melting species is inverted gate by gate
        # through the reference's linear interpolator over (V(D_k), D_k), hydrometeors.py:480-500 -- cpol_spectrum.inl)
        spectrum = conf['doppler']['scheme'] == 3
        key = (scheme, conf['radar']['frequency'], conf['microphysics']['scattering'], tuple(hl),
               conf['doppler']['scheme'] == 2, spectrum)
        cache = self.__dict__.setdefault('_lut_cache', {})
        if key in cache:
            # tables of a configuration seen before (e.g. the Ku / Ka / ground switches of
            # get_GPM_swath): no file reads, no per-bin factor rebuild -- only the H2D staging
            lut, built = cache[key]
            self.lut_sz = lut
            self._drop_lanes()
            self._stage_t_functions(hl, scheme)
            for slot, h in enumerate(hl):
                d, table, pre, dnu, aux, dw, st = built[h]
                self._ctx.stage_hydro(slot, d, table, pre, dnu, aux)
                if dw is not None:
                    self._ctx.stage_doppler_weights(slot, dw)
                if st is not None:
                    self._ctx.stage_spectrum_tables(slot, *st)
            self._ctx.set_num_hydro(len(hl))
            self._ctx.prepare()                  # integral tables of this table set (cpol_prepare)
            self._staged_hydro = hl
            if self._model_staged and self._staged_vars != hyd.variable_list(conf):
                self._stage_model()
            return
        if callable(self._user_luts):
            lut = self._user_luts(hl, conf['radar']['frequency'], scheme)
        elif self._user_luts is not None:
            missing = [h for h in hl if h not in self._user_luts]
            if missing:
                raise IOError('no lookup table supplied for hydrometeors %s' % missing)
            lut = {h: self._user_luts[h] for h in hl}
        else:
            lut = load_all_lut(scheme, hl, conf['radar']['frequency'],
                               conf['microphysics']['scattering'], lut_dir=self.lut_dir)
        self.lut_sz = lut
        self._drop_lanes()
        self._stage_t_functions(hl, scheme)
        var_index = {v: i for i, v in enumerate(hyd.variable_list(conf))}
        built = {}
        for slot, h in enumerate(hl):
            d, table, pre, dnu, aux = hyd.build_hydro(h, scheme, lut[h], var_index)
            # identity of this slot's content for the library's integral-table cache: the table
            # set is kept alive (and unchanged) by _lut_cache below
            d.table_id = _table_identity() if len(cache) < 4 else 0
            self._ctx.stage_hydro(slot, d, table, pre, dnu, aux)
            dw = None
            if conf['doppler']['scheme'] == 2:
                dw = hyd.doppler_weights(h, scheme, lut[h])
                self._ctx.stage_doppler_weights(slot, dw)
            st = None
            if spectrum:
                st = hyd.spectrum_tables(h, scheme, lut[h])
                self._ctx.stage_spectrum_tables(slot, *st)
            built[h] = (d, table, pre, dnu, aux, dw, st)
        if len(cache) < 4:                       # a few table sets at most (host memory)
            cache[key] = (lut, built)
        self._ctx.set_num_hydro(len(hl))
        self._ctx.prepare()                      # integral tables of this table set (cpol_prepare)
        self._staged_hydro = hl
        if self._model_staged and self._staged_vars != hyd.variable_list(conf):
            self._stage_model()                 # variable set changed (1mom <-> 2mom)

    def _stage_t_functions(self, hl, scheme):
        """Host-tabulated float32 functions of the temperature (1-moment snow intercept, 1-moment
        ice moment relation): staged once per context, only when the species is simulated."""
        if scheme != '1mom':
            return
        done = self.__dict__.setdefault('_tfun_staged', set())
        want = [(n, w) for n, w, h in (('snow_n0', N.TFUN_SNOW_N0, 'S'), ('ice_mom2_a', N.TFUN_ICE_MOM2_A, 'I'))
                if (h in hl or (h == 'S' and 'mS' in hl)) and n not in done]
        if not want:
            return
        tabs = hyd.t_function_tables([n for n, _ in want])
        for n, w in want:
            self._ctx.stage_t_function(w, tabs[n])
            done.add(n)

    # ------------------------------------------------------------------ model
    def load_model_file(self, filename, cfilename=None):
        """Loads the model variables from a file (cosmo_pol/radar_operator.py:217-309): GRIB edition 1 as COSMO writes
        it (cosmo_pol_amd/grib1.py; names through `self.grib_table`), NetCDF classic in COSMO's conventions or an .npz
        archive with the same names (cosmo_pol_amd/model_io.py), the c-file `cfilename` supplying the half-level
        heights HHL when the file has none.  The file may hold the raw model output (P, T, QV, QR, QC, QI, QS, QG, U,
        V, W [+ QH, QNH, QNR, QNS, QNG]), from which the densities, RHO and -- for refraction scheme 2 -- the
        refractivity N are derived as pycosmo does for the reference, or the derived variables themselves.
        A GRIB-1 file of raw output whose heights come from itself or from a GRIB-1 c-file is unpacked, derived and
        staged on the GPU (the packed octets travel as they are; `dic_vars[...].data`, `N.data` and the level heights
        are then decoded on the host only when read); every other combination goes through the host
        (model_io.read_model_file).  Both ways stage the same bits for the configuration in force.  One difference
        afterwards: the device path keeps the file's index, so an `EDR` in the file is staged when
        `doppler/turbulence_correction` is switched on later; the host path read `EDR` only if the correction was on at
        load time and otherwise switches it off again with the reference's notice.  ValueError when a necessary variable
        is missing, as in the reference (:264-275).  A file that is refused (NotImplementedError, ValueError) leaves
        the operator and its staged cube as they were; after a device error during the ingest no model is staged."""
        from . import model_io
        want_n = self.__config['refraction']['scheme'] == 2
        packed = self._open_packed(filename, cfilename)
        if packed is not None:
            self._load_model_packed(packed[0], packed[1], want_n)
            print('-------done------')
            return
        m = model_io.read_model_file(filename, cfilename, want_refractivity=want_n, want_edr=self._wants_edr(),
                                     grib_table=self.grib_table)
        if want_n and 'N' not in m['data']:
            # (radar_operator.py:237-247)
            print('Necessary variables for computation of atm. refractivity were not found in file. '
                  'Using 4/3 method instead.')
        print('Using %s scheme' % ('2-moment' if m['scheme'] == '2mom' else '1-moment'))
        print('Reading variables ', sorted(m['data']), ' from file')
        self.load_model_arrays(m['data'], m['zlevels'], m['proj_info'], m['resolution'], time=m['time'])
        print('-------done------')

    # (the device ingest of GRIB-1 files)
    @staticmethod
    def _is_grib1(path):
        if path is None or not os.path.exists(path):
            return False
        with open(path, 'rb') as f:
            magic = f.read(8)
        return len(magic) == 8 and magic[:4] == b'GRIB' and magic[7] == 1

    def _open_packed(self, filename, cfilename):
        """(model source, c-file source | None) when the files take the device path, else None (host path).  The choice
        follows from the files alone: a GRIB-1 file of raw output with HHL in itself or in a GRIB-1 c-file."""
        from . import model_io
        if not self._is_grib1(filename):
            return None
        g = model_io._Grib1(filename, self.grib_table)
        c = None
        try:
            names = g.names()
            if all(k in names for k in model_io.BASE_VARIABLES) or not all(k in names for k in model_io.RAW_BASE) \
                    or 'z-levels' in names:
                g.close()
                return None                      # (derived variables, or the host path's ValueError naming what is missing)
            if 'HHL' not in names:
                if not self._is_grib1(cfilename):
                    g.close()
                    return None
                c = model_io._Grib1(cfilename, self.grib_table)
                if 'HHL' not in c.names():
                    c.close()
                    g.close()
                    return None
            return g, c
        except BaseException:
            g.close()
            if c is not None:
                c.close()
            raise

    def _drop_packed(self):
        p, self._packed = getattr(self, '_packed', None), None
        if p is not None:
            p['g'].close()
            if p['c'] is not None:
                p['c'].close()

    @property
    def _zlevels(self):
        if self._zl is None and self._packed is not None:
            self._zl = self._packed_host()['zlevels']
        return self._zl

    @_zlevels.setter
    def _zlevels(self, value):
        self._zl = value

    def _packed_host(self):
        """The host decode of the files ingested on the device (model_io.read_model_file on the open sources), once."""
        from . import model_io
        p = self._packed
        if p['host'] is None:
            p['host'] = model_io.read_model_file(p['g'], p['c'], want_refractivity=p['want_n'], want_edr=True)
        return p['host']

    def _load_model_packed(self, g, c, want_n):
        """Checks of model_io.read_model_file on the index alone, then the operator's state as load_model_arrays leaves
        it -- with lazily decoded arrays -- and the device ingest (_stage_model).  Raises before anything changes."""
        from . import model_io
        try:
            G, H = g.g, (g if c is None else c).g
            names = G.names()
            nz = G.n_levels('T')
            two_mom = all(k in names for k in model_io.RAW_2MOM)
            raw = model_io.RAW_BASE + ([k for k in model_io.RAW_2MOM + ['QNI'] if k in names] if two_mom else [])
            for k in raw + (['EDR'] if 'EDR' in names else []):
                n = G.n_levels(k)
                if n != nz and not (k in ('W', 'EDR') and n == nz + 1):
                    raise ValueError('variable %s has %d levels, T has %d' % (k, n, nz))
            if H.n_levels('HHL') not in (nz, nz + 1) or H.shape() != G.shape():
                raise ValueError('level heights have shape %s, the variables %s'
                                 % ((H.n_levels('HHL'),) + H.shape(), (nz,) + G.shape()))
            top, low = H.get('HHL', levels=(0, H.n_levels('HHL') - 1))
            if top.mean() < low.mean():
                raise ValueError('level 0 must be the model top (heights decreasing with the level index)')
            ny, nx = G.shape()
            proj = G.proj_info()
            res = ((proj['Lo2'] - proj['Lo1']) / max(nx - 1, 1), (proj['La2'] - proj['La1']) / max(ny - 1, 1))
            time = G.time()
        except BaseException:
            g.close()
            if c is not None:
                c.close()
            raise
        keys = list(hyd.BASE_VARIABLES) + (list(hyd.BASE_VARIABLES_2MOM) if two_mom else []) + (['EDR'] if 'EDR' in names else [])
        print('Using %s scheme' % ('2-moment' if two_mom else '1-moment'))
        print('Reading variables ', sorted(keys + (['N'] if want_n else [])), ' from file')
        self._note_missing_edr('EDR' in keys)
        previous = (self._packed, self.dic_vars, self.N, self._zl, getattr(self, '_proj', None), getattr(self, '_res', None))
        self._packed = {'g': g, 'c': c, 'two_mom': two_mom, 'want_n': want_n, 'host': None, 'nz': nz}
        attrs = LazyDict()
        attrs.add('z-levels', lambda: self._zlevels)
        attrs['proj_info'], attrs['resolution'], attrs['time'] = proj, (float(res[0]), float(res[1])), time
        host = self._packed_host
        self.dic_vars = {k: LazyModelVar(k, lambda k=k: host()['data'][k], attrs) for k in keys}
        self.N = LazyModelVar('N', lambda: host()['data']['N'], attrs) if want_n else 0
        self._zl = None
        try:
            self._adopt_model(proj, attrs['resolution'], two_mom)
        except BaseException as e:
            g.close()
            if c is not None:
                c.close()
            self._packed, self.dic_vars, self.N, self._zl, self._proj, self._res = previous
            if not isinstance(e, ValueError):
                # (CPOL_ERR_ARG -- ValueError -- is raised before the library changes anything: the operator keeps the cube
                # it had; after anything else the library holds no staged model)
                self._model_staged = False
            raise
        if previous[0] is not None:
            previous[0]['g'].close()
            if previous[0]['c'] is not None:
                previous[0]['c'].close()

    def _wants_edr(self):
        """The eddy dissipation rate is a model variable only for the turbulence broadening of the Doppler spectrum
        (radar_operator.py:251-254)."""
        d = self.__config['doppler']
        return d['scheme'] == 3 and d['turbulence_correction'] == 1

    def load_model_arrays(self, data, zlevels, proj_info, resolution, time=None):
        """data: {name: [nz, ny, nx] float32} with the names of the reference
        (U, V, W, QR_v, QS_v, QG_v, QI_v, RHO, T [+ QH_v, QN*_v] [+ EDR]); zlevels
        [nz, ny, nx] (level 0 = model top); proj_info with Lo1, La1, Lo2, La2,
        Latitude_of_southern_pole, Longitude_of_southern_pole; resolution
        (dlon, dlat).  EDR (eddy dissipation rate) is staged only with Doppler scheme 3 and
        doppler/turbulence_correction = 1; without it that correction is switched off with the reference's notice."""
        self._note_missing_edr('EDR' in data)
        two_mom = all(k in data for k in hyd.BASE_VARIABLES_2MOM)
        missing = [k for k in hyd.BASE_VARIABLES if k not in data]
        if missing:
            raise ValueError('Not all necessary variables could be found: missing %s' % missing)
        attrs = {'z-levels': zlevels, 'proj_info': proj_info, 'resolution': resolution,
                 'time': time}
        self._drop_packed()
        self.dic_vars = {k: ModelVar(k, v, attrs) for k, v in data.items() if k != 'N'}
        self.N = ModelVar('N', data['N'], attrs) if 'N' in data else 0     # refractivity
        self._zlevels = zlevels
        self._adopt_model(proj_info, resolution, two_mom)

    def _note_missing_edr(self, have_edr):
        if self._wants_edr() and not have_edr:
            # (radar_operator.py:255-262: the reference edits its configuration in the same way)
            print('Necessary variable for correction of turbulence broadening: Eddy dissipitation rate '
                  'was not found in file. No  turbulence correction will be done.')
            self.__config['doppler']['turbulence_correction'] = 0
            self._cache = {}

    def _adopt_model(self, proj_info, resolution, two_mom):
        scheme = '2mom' if two_mom else '1mom'
        self._proj = proj_info
        self._res = resolution
        if scheme != self.__config['microphysics']['scheme']:
            print('Using %s scheme' % ('2-moment' if two_mom else '1-moment'))
            conf = self.config
            conf['microphysics']['scheme'] = scheme
            self._model_staged = False
            self.config = conf
        self._stage_model()

    def _stage_model(self):
        conf = self.__config
        self._drop_lanes()
        names = hyd.variable_list(conf)
        if self._wants_edr() and 'EDR' in self.dic_vars:
            names = names + ['EDR']            # last: the indices of every other variable stay what they are without it
        p = self._proj
        llc = np.asarray((float(p['Lo1']), float(p['La1']))).astype('float32')
        urc = np.asarray((float(p['Lo2']), float(p['La2']))).astype('float32')
        res = np.asarray(self._res, dtype=np.float32)
        sp = [float(p['Latitude_of_southern_pole']), float(p['Longitude_of_southern_pole'])]
        if self._packed is not None:
            self._ctx.stage_model_packed(*self._packed_plan(names, llc, urc, res, sp))
        else:
            self._ctx.stage_model([self.dic_vars[n].data for n in names], self._zlevels, llc, urc,
                                  res, sp)
        self._staged_vars = names
        self._model_staged = True
        self._staged_serial = getattr(self, '_staged_serial', 0) + 1      # (host caches that depend on the cube)
        # (a freshly staged cube is alone: the library dropped the members that lay beside the previous one)
        self._n_members, self._member = 1, 0

    def _packed_plan(self, names, llc, urc, res, sp):
        """(cpol_packed_model, planes) of the device ingest for the staged variables `names`: the raw fields each of them
        needs and its recipe -- the statements of model_io.derive and read_model_file."""
        from . import model_io
        pk = self._packed
        G, H, nz = pk['g'].g, (pk['g'] if pk['c'] is None else pk['c']).g, pk['nz']
        have = G.names()
        fields = []                               # (file, raw name)

        def field(name, src=G):
            if (src, name) not in fields:
                fields.append((src, name))
            return fields.index((src, name))

        m = N.PackedModel()
        m.nz, (m.ny, m.nx) = nz, G.shape()
        m.field_p, m.field_t, m.field_qv, m.field_hhl = field('P'), field('T'), field('QV'), field('HHL', H)
        load = [k for k in ('QC', 'QR', 'QS', 'QG', 'QI') if k in have]
        m.n_load = len(load)
        for j, k in enumerate(load):
            m.field_load[j] = field(k)
        m.n_vars = len(names)
        for v, name in enumerate(names):
            if name == 'RHO':
                m.recipe[v] = N.RECIPE_RHO
            elif name.endswith('_v'):
                rawname = name[:-2]
                if rawname in have:
                    m.recipe[v], m.source[v] = N.RECIPE_TIMES_RHO, field(rawname)
                else:
                    m.recipe[v] = N.RECIPE_ZEROS
            else:
                half = G.n_levels(name) == nz + 1
                m.recipe[v], m.source[v] = (N.RECIPE_HALF_MEAN if half else N.RECIPE_COPY), field(name)
        if len(fields) > N.MAX_RAW_FIELDS:
            raise ValueError('more than %d raw fields' % N.MAX_RAW_FIELDS)
        m.n_fields = len(fields)
        m.r_d, m.rv_rd_m1 = model_io.R_D, model_io.R_V / model_io.R_D - 1.0
        m.llc[:], m.urc[:], m.res[:], m.south_pole[:] = list(llc), list(urc), list(res), list(sp)
        planes = []
        octets = {}
        for f, (src, name) in enumerate(fields):
            if src not in octets:
                octets[src] = np.frombuffer(src.buf, dtype=np.uint8)
            pl = src.planes(name)
            m.field_levels[f] = len(pl)
            for k, e in enumerate(pl):
                planes.append((octets[src][e['data_offset']:e['data_offset'] + e['n_octets']], e['R'], e['E'], e['D'],
                               e['n_bits'], e['scanning'] == 0x00, f, k))
        return m, planes

    def get_pos_and_time(self):
        c = self.__config['radar']['coords']
        t = None
        if self.dic_vars:
            t = self.dic_vars['T'].attributes.get('time')
        return {'latitude': c[0], 'longitude': c[1], 'altitude': c[2], 'time': t}

    # ------------------------------------------------------------------ sweeps
    def _check_ready(self):
        if not self.dic_vars or not self._model_staged:
            print('No model file has been loaded! Aborting...')
            return False
        return True

    def simulate_rays(self, azimuths, elevations, on_device=False, device_outputs=None,
                      apply_sensitivity=True, paths=None, lane=0, pinned=False):
        """One batched launch sequence for the given rays (az[i], el[i]) of the
        ground radar of the configuration.  Returns a dict of [n_rays, n_gates]
        arrays (linear units, NaN = no data).
        `device_outputs`: optional {field: device pointer} (outputs stay in HBM).
        `paths`: optional float32 [n_rays, n_vnodes, 3, n_gates] host-computed ray
        paths (s, h, e_deg) replacing the 4/3-earth model (CPOL_GEOM_HOST_PATHS).
        `lane`: which forked context (stream + work buffers) runs the sweep; sweeps on
        different lanes overlap on the GPU (one host thread per lane at a time).
        Host outputs are views of one block of page-locked memory from the operator's pool,
        filled by a single device-to-host copy queued behind the kernels; the block stays theirs
        until the last of them is dropped (then it is re-used by a later sweep).
        `pinned`: do not wait -- the call returns once the sweep is queued; call `wait(lane)` before
        reading the arrays.  (The copy of one sweep then overlaps the kernels of the sweeps on the
        other lanes.)  The gate coordinates (`lats`, `lons`, `dist`, `heights`) of an unchanged
        scan geometry are read-only arrays shared between results."""
        return self._simulate_rays(azimuths, elevations, device_outputs=device_outputs, apply_sensitivity=apply_sensitivity,
                                   paths=paths, lane=lane, pinned=pinned)

    def simulate_rays_superob(self, azimuths, elevations, superob, keep_gates=False, rays_per_block=0, device_outputs=None,
                              apply_sensitivity=True, paths=None, lane=0, pinned=False):
        """simulate_rays handing back SUPEROBSERVATIONS: `superob` is a superob.Superob, and the result gains res['superob'] --
        the window averages of the radar fields made on the device behind the sweep (superob.average states the rule;
        [window rows, window columns] arrays), 'count' {field: uint16 array} and the window means of lats, lons, dist,
        heights.  Without `keep_gates` the per-gate radar fields, the mask and -- with output_variables='all' -- the
        antenna-integrated model variables (`model_vars`: not averaged, and per gate like the rest) are neither produced for
        the host nor copied (the result keeps the shared gate coordinates); with it all arrive, with the bits of simulate_rays.
        `rays_per_block`: windows do not cross blocks of that many rays (0: all rays of the call; the rays of one sweep when
        the call holds several).  With `device_outputs`: its entry 'superob' is {field or 'count': device pointer}.
        The other keywords: as for simulate_rays.  (A method of its own: the keyword list of simulate_rays is pinned.)
        NotImplementedError with a process group (windows would cross the ray shards) and for spaceborne geometry."""
        return self._simulate_rays(azimuths, elevations, device_outputs=device_outputs, apply_sensitivity=apply_sensitivity,
                                   paths=paths, lane=lane, pinned=pinned,
                                   product=SO.Windows(superob, keep_gates, rays_per_block, self.distributed))

    def simulate_rays_moments(self, azimuths, elevations, moments, keep_spectrum=False, device_outputs=None,
                              apply_sensitivity=True, paths=None, lane=0, pinned=False):
        """simulate_rays handing back SPECTRUM MOMENTS (Doppler scheme 3): `moments` is a spectrum_moments.SpectrumMoments,
        and the result gains res['moments'] -- {field: float64 [n_rays, n_gates]} for its fields and 'count' (uint16, the
        bins that counted), made on the device behind the sweep from the spectrum as the call delivers it
        (spectrum_moments.moments states the rule).  Without `keep_spectrum` DSPECTRUM is neither produced for the host nor
        copied and its key is absent; with it the result carries every array of simulate_rays, bit for bit.  With
        `device_outputs`: its entry 'moments' is {'moments': device pointer of [8, n_rays, n_gates] float64 (only the rows of
        the requested fields are written), 'count': device pointer}.  The other keywords: as for simulate_rays.  (A method
        of its own: the keyword list of simulate_rays is pinned.)  ValueError when the configured Doppler scheme is not 3;
        NotImplementedError with a process group and for spaceborne geometry."""
        return self._simulate_rays(azimuths, elevations, device_outputs=device_outputs, apply_sensitivity=apply_sensitivity,
                                   paths=paths, lane=lane, pinned=pinned,
                                   product=SM.Rows(moments, keep_spectrum, self.__config['doppler']['scheme'], self.distributed))

    def _simulate_rays(self, azimuths, elevations, device_outputs=None, apply_sensitivity=True, paths=None, lane=0, pinned=False,
                       product=None, radar=None, source=0):
        conf = self.__config
        coords = conf['radar']['coords'] if radar is None else self._radar_arg(radar)
        if coords[2] > K.MAX_MODEL_HEIGHT:
            raise NotImplementedError('spaceborne geometry: use get_GPM_swath')
        rr = self.constants.RANGE_RADAR
        if conf['refraction']['scheme'] == 2 and paths is None:
            if self.N is None or isinstance(self.N, int):
                # reference: falls back to the 4/3 model with a notice
                # (interpolation.py:138-145, radar_operator.py:237-247)
                print('Refraction scheme 2 needs the refractivity N as an additional model '
                      'variable; 4/3 Earth model will be used instead...')
            else:
                from . import refraction
                sub = self._cached('sub', lambda: quadrature.subbeams(conf))
                h_col, n_col = refraction.refractivity_column(
                    self.N.data, self._zlevels, self._proj, self._res, coords,
                    conf['radar'].get('type', 'ground'))
                paths = refraction.ode_paths(rr, elevations, sub.pts_ver, coords, h_col, n_col)
        mode = N.GEOM_GROUND_43 if paths is None else N.GEOM_HOST_PATHS
        if product is not None and hasattr(product, 'set_plane'):
            self._set_plane(product, azimuths, elevations, coords, paths, source, device_outputs, lane)
        return self._run_rays(azimuths, elevations, coords, len(rr), float(rr[0]), mode,
                              device_outputs=device_outputs, apply_sensitivity=apply_sensitivity,
                              paths=paths, lane=lane, pinned=pinned, product=product)

    @staticmethod
    def _radar_arg(radar):
        """`radar=` of a composite call: (lat, lon, alt) in place of config['radar']['coords'] for this call alone."""
        c = np.asarray(radar, dtype=np.float64).reshape(-1)
        if c.size != 3 or not np.all(np.isfinite(c)):
            raise ValueError('radar: (latitude, longitude, altitude), three finite numbers, got %r' % (radar,))
        return [float(v) for v in c]

    def _ray_tables(self, az, el, coords, sub):
        """(version, traj, geo) of a set of rays: per-ray tables depend only on (site, azimuths, elevations, quadrature nodes);
        `version` lets the library keep its device copies when they did not change."""
        key = ('rays', az.tobytes(), el.tobytes(), tuple(np.ravel(coords)))

        def make():
            RadarOperator._table_serial += 1
            return (RadarOperator._table_serial,) + geo.ray_tables(coords, az, el, sub)
        return self._cached(key, make, lru=32)      # (the sweeps of a network of radars: 3 radars x 5 elevations are 15 sets)

    def _set_plane(self, product, azimuths, elevations, coords, paths, source, device_outputs, lane):
        """Hands a composite product the part of a network composite that belongs to THIS call: its `source`, and on a plane other
        than 'radar' the per-gate coordinates of the call's rays (composite.plane_xy of the gate coordinates `lats` / `lons`).
        Of a table set with a version tag they are made once and cached beside the geometry (('geom', version, n_gates)),
        read-only, under a plane_version of their own, so that the library keeps its device copy too.  When the table set's gate
        coordinates are not cached yet they are fetched first: the first time a geometry is seen costs ONE plain call on `lane`.
        Without a version tag (host ray paths, reuse_device_tables off) that plain call is made every time and plane_version is 0.
        With device outputs the caller brings device pointers (device_outputs['composite']['gate_x' | 'gate_y'])."""
        cspec = getattr(product, 'maps', product).spec
        if not cspec.gate_plane or device_outputs is not None:
            product.set_plane(None, 0, source)
            return
        conf = self.__config
        az = np.ascontiguousarray(np.asarray(azimuths, dtype=np.float64).reshape(-1))
        el = np.ascontiguousarray(np.asarray(elevations, dtype=np.float64).reshape(-1))
        if az.shape != el.shape:
            raise ValueError('azimuths and elevations must have the same length')
        rr = self.constants.RANGE_RADAR
        n_gates = len(rr)
        pole = None
        if cspec.plane == 'model':
            if not self._model_staged:
                raise ValueError("the plane 'model' needs a loaded model")
            pole = (float(self._proj['Latitude_of_southern_pole']), float(self._proj['Longitude_of_southern_pole']))
        version = 0
        if paths is None and self.reuse_device_tables:
            sub = self._cached('sub', lambda: quadrature.subbeams(conf))
            version = self._ray_tables(az, el, coords, sub)[0]
        pkey = ('plane', version, n_gates, cspec.plane, pole)
        made = self._cache.get(pkey) if version else None
        if made is None:
            geom = self._cache.get(('geom', version, n_gates)) if version else None
            if geom is None:
                geom = self._run_rays(az, el, coords, n_gates, float(rr[0]), N.GEOM_GROUND_43 if paths is None else N.GEOM_HOST_PATHS,
                                      paths=paths, lane=lane)
            x, y = CP.plane_xy(cspec.plane, geom['lats'], geom['lons'], pole)
            if version:
                x, y = x.copy(), y.copy()         # (own read-only copies: shared by every later call of this table set)
                x.flags.writeable = y.flags.writeable = False
                def tagged():
                    RadarOperator._plane_serial += 1
                    return (RadarOperator._plane_serial, x, y)
                made = self._cached(pkey, tagged, lru=32)
            else:
                made = (0, x, y)
        product.set_plane((made[1], made[2]), made[0], source)

    def stencil_state(self, lane=0):
        """The gate stencils as the library reports them: 'form' of the last sweep on `lane` (0 full, 1 recording, 2 replay) and the
        store's 'entries', 'bytes', 'records', 'replays', 'drops'."""
        return self._lane(lane).stencil_state()

    def wait(self, lane=0):
        """Waits for the sweeps queued on `lane` (pinned / device outputs); raises IndexError
        if one of them left the model domain."""
        self._lane(lane).synchronize()

    # ------------------------------------------------------------------ per-radial seam
    def _column_names(self):
        """Variable order of the columns: the staged model's, or the configuration's when no model is loaded (with the
        turbulence broadening of the Doppler spectrum: followed by EDR)."""
        if self._model_staged:
            self._sync_edr()
            return list(self._staged_vars)
        return hyd.variable_list(self.__config) + (['EDR'] if self._wants_edr() else [])

    def _sync_edr(self):
        """EDR is staged exactly when the configuration in force broadens by turbulence: a configuration set after the
        model was loaded restages the cube, or switches the correction off when the model has no EDR."""
        want = self._wants_edr()
        if want and 'EDR' not in self.dic_vars:
            print('Necessary variable for correction of turbulence broadening: Eddy dissipitation rate '
                  'was not found in file. No  turbulence correction will be done.')
            self.__config['doppler']['turbulence_correction'] = 0
            self._cache = {}
            want = False
        if want != ('EDR' in self._staged_vars):
            self._stage_model()

    def _fill_broadening(self, p, names, range0):
        """The broadening fields of cpol_sweep_params for a scheme-3 launch (doppler_scatter.py:360-369, 727-777): the
        constants as the reference's statements give them."""
        conf = self.__config
        turb = bool(conf['doppler']['turbulence_correction']) and 'EDR' in names
        motion = bool(conf['doppler']['motion_correction'])
        if not (turb or motion):
            return
        bw = conf['radar']['3dB_beamwidth']
        va = self.constants.VARRAY
        p.turbulence_correction, p.motion_correction = int(turb), int(motion)
        p.var_edr = names.index('EDR') if turb else -1
        p.range0 = range0
        p.sigma_r = float(0.35 * conf['radar']['radial_resolution'])
        p.sigma_theta = float(np.deg2rad(bw) / (4. * np.sqrt(np.log(2))))
        p.motion_num = float(self.constants.WAVELENGTH / 100. * conf['radar']['antenna_speed'])
        p.motion_den = float(2 * np.pi * np.deg2rad(bw))
        p.v_res = float(va[2] - va[1])

    def interpolate_rays(self, azimuths, elevations, melting=True, on_device=False, lane=0):
        """The first half of simulate_rays (cpol_interp_subbeams): the sub-beam columns of the rays (az[i], el[i]) as the
        reference's get_interpolated_radial leaves them (interpolation/interpolation.py:91, melting.py:19-90), for all
        rays at once.  Returns the dict simulate_columns takes: [n_rays, n_sub, n_gates] arrays -- one per model variable,
        'mask' (int8 codes), 'elev' (not folded), 'lats', 'lons', 'dist', 'heights' of every sub-beam and, with the
        melting scheme, 'QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG', 'mask_ml' and 'has_melting' [n_rays, n_sub] -- plus
        'quad_pts' [n_rays, n_sub, 2] (azimuth, elevation) and 'quad_weights' ([n_sub]; per gate under integration scheme
        'ml').  The values carry the bits simulate_rays scatters.  `melting`: apply the melting scheme when the
        configuration melts (False: raw values; simulate_columns then melts on the device).  `on_device`: torch tensors
        on the operator's GPU, ordered before torch's current stream."""
        if not self._check_ready():
            raise ValueError('interpolate_rays: no model loaded')
        conf = self.__config
        coords = conf['radar']['coords']
        if coords[2] > K.MAX_MODEL_HEIGHT:
            raise NotImplementedError('spaceborne geometry: use get_GPM_swath')
        rr = self.constants.RANGE_RADAR
        paths = None
        if conf['refraction']['scheme'] == 2 and not (self.N is None or isinstance(self.N, int)):
            from . import refraction
            sub = self._cached('sub', lambda: quadrature.subbeams(conf))
            h_col, n_col = refraction.refractivity_column(self.N.data, self._zlevels, self._proj, self._res, coords,
                                                          conf['radar'].get('type', 'ground'))
            paths = refraction.ode_paths(rr, elevations, sub.pts_ver, coords, h_col, n_col)
        mode = N.GEOM_GROUND_43 if paths is None else N.GEOM_HOST_PATHS
        return self._run_rays(azimuths, elevations, coords, len(rr), float(rr[0]), mode, apply_sensitivity=False,
                              paths=paths, lane=lane, subbeams={'melting': bool(melting), 'on_device': bool(on_device)})

    def _export_subbeams(self, p, t, keep, sub, az, el, n_gates, lane, melting, on_device):
        conf = self.__config
        names = list(self._staged_vars)
        n_rays, n_sub = len(az), sub.n_sub
        shape = (n_rays, n_sub, n_gates)
        melt = melting and bool(conf['microphysics']['with_melting'])
        ml = sub.sub_smooth is not None
        spec = [('vals', np.float32, (len(names),) + shape), ('mask', np.int8, shape), ('elev', np.float32, shape),
                ('lats', np.float64, shape), ('lons', np.float64, shape), ('dist', np.float32, shape),
                ('heights', np.float32, shape)]
        if melt:
            spec += [('q_melt', np.float32, (2,) + shape), ('fw_melt', np.float64, (2,) + shape), ('mask_ml', np.int8, shape)]
        if ml:
            spec.append(('wgate', np.float64, shape))
        ctx = self._lane(lane)
        so = N.SubbeamOutputs()
        so.skip_melting = int(not melt)
        so.outputs_on_device = int(bool(on_device))
        if on_device:
            import torch
            dev = torch.device('cuda', self.device)
            arrs = {k: torch.empty(sh, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, dt, sh in spec}
            for k, a in arrs.items():
                setattr(so, k, a.data_ptr())
            ext = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
            ext.wait_stream(torch.cuda.current_stream(dev))
            ctx.interp_subbeams(p, t, so)
            torch.cuda.current_stream(dev).wait_stream(ext)
        else:
            arrs = {k: np.empty(sh, dtype=dt) for k, dt, sh in spec}
            for k, a in arrs.items():
                setattr(so, k, a.ctypes.data)
            ctx.interp_subbeams(p, t, so)
        del keep
        out = {nm: arrs['vals'][i] for i, nm in enumerate(names)}
        for k in ('mask', 'elev', 'lats', 'lons', 'dist', 'heights'):
            out[k] = arrs[k]
        if melt:
            out['QmS_v'], out['QmG_v'] = arrs['q_melt'][0], arrs['q_melt'][1]
            out['fwet_mS'], out['fwet_mG'] = arrs['fw_melt'][0], arrs['fw_melt'][1]
            out['mask_ml'] = arrs['mask_ml']
            out['has_melting'] = arrs['mask_ml'].any(-1) if not on_device else arrs['mask_ml'].bool().any(-1)
        # (the angles of geometry.ray_tables: node + ray, the same float64 sums)
        pts = np.stack([sub.pts_hor[sub.sub_h][None, :] + az[:, None], sub.pts_ver[sub.sub_v][None, :] + el[:, None]],
                       axis=-1)
        out['quad_pts'] = np.ascontiguousarray(pts)
        out['quad_weights'] = arrs['wgate'] if ml else np.array(sub.sub_w, dtype=np.float64)
        return out

    def get_interpolated_radial(self, azimuth, elevation):
        """The reference's get_interpolated_radial (interpolation/interpolation.py:91) on the GPU: one Radial per kept
        sub-beam of the ray (azimuth, elevation), with `values` (the model variables and, when the configuration melts,
        QmS_v, QmG_v, fwet_mS, fwet_mG), `mask`, the lats / lons / dist / heights / elev profiles, `quad_pt`,
        `quad_weight`, `has_melting` and `mask_ml`."""
        from .radial import Radial
        c = self.interpolate_rays([azimuth], [elevation], melting=True)
        names = list(self._staged_vars) + [k for k in ('QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG') if k in c]
        w = c['quad_weights']
        out = []
        for s in range(c['elev'].shape[1]):
            values = {k: (c[k][0, s].astype(np.float64) if k in ('QmS_v', 'QmG_v') else c[k][0, s]) for k in names}
            r = Radial(values, c['mask'][0, s].astype(np.float64), c['lats'][0, s], c['lons'][0, s], c['dist'][0, s],
                       c['heights'][0, s], elev_profile=c['elev'][0, s], quad_pt=[float(x) for x in c['quad_pts'][0, s]],
                       # (a NumPy float64 as the reference's `weights[i, j]`: integrate_radials then forms the float32 values'
                       # products in float64, interpolation.py:60-75; a Python float would leave them in float32)
                       quad_weight=(w[0, s] if np.ndim(w) == 3 else np.float64(w[s])))
            if 'mask_ml' in c:
                r.mask_ml = c['mask_ml'][0, s].astype(bool)
                r.has_melting = bool(c['has_melting'][0, s])
            out.append(r)
        return out

    def simulate_columns(self, columns, apply_sensitivity=False, device_outputs=None, lane=0, pinned=False):
        """The second half of simulate_rays on caller-supplied sub-beam columns (cpol_run_columns): what the
        reference's get_radar_observables + integrate_radials do for every radial (doppler_scatter.py:49-489).
        `columns`: dict of [n_rays, n_sub, n_gates] arrays -- one per model variable of the configuration (the names
        of simulate_rays' model_vars), 'elev' (degrees, unfolded or folded), optionally 'mask' (codes), the given melting
        fields 'QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG' (then the variables are the melted ones, as the reference's
        sub-radials carry them) with 'has_melting' [n_rays, n_sub], and 'lats', 'lons', 'dist', 'heights' (the central
        sub-beam's become the result's geometry) -- plus 'quad_pts' [n_rays, n_sub, 2] (azimuth, elevation in degrees)
        and 'quad_weights' [n_sub] (per-gate [n_rays, n_sub, n_gates] for integration scheme 'ml').  NumPy arrays or
        torch tensors on the operator's GPU (read in place after torch's current stream; never written).
        Works without a loaded model.  Returns the dict of simulate_rays.
        Terrain shadowing (integration/terrain_shadow) is NOT applied here: the caller's masks stand (cosmo_pol_amd.shadow.apply
        shadows columns of interpolate_rays(melting=False) on the host).  With integration/terrain_visibility the result
        carries 'visibility' of the masks as they came."""
        conf = self.__config
        names = self._column_names()
        missing = [k for k in names + ['elev', 'quad_pts', 'quad_weights'] if k not in columns]
        if missing:
            raise ValueError('simulate_columns: missing %s' % missing)
        elev = columns['elev']
        if len(tuple(elev.shape)) != 3:
            raise ValueError('simulate_columns: columns must be [n_rays, n_sub, n_gates] arrays')
        n_rays, n_sub, n_gates = (int(x) for x in elev.shape)
        torch_in = _is_torch(elev)
        keep = []

        def per_gate(name, dtype, shape=(n_rays, n_sub, n_gates), required=True):
            a = columns.get(name)
            if a is None:
                if required:
                    raise ValueError('simulate_columns: missing %s' % name)
                return None
            if tuple(a.shape) != tuple(shape):
                raise ValueError('simulate_columns: %s has shape %s, expected %s' % (name, tuple(a.shape), tuple(shape)))
            if _is_torch(a) != torch_in:
                raise ValueError('simulate_columns: mixed torch / NumPy columns (%s)' % name)
            if torch_in:
                import torch
                if a.device.type != 'cuda' or a.device.index != self.device:
                    raise ValueError('simulate_columns: %s is not on the operator\'s GPU' % name)
                a = a.to(getattr(torch, np.dtype(dtype).name)).contiguous()
                keep.append(a)
                return a.data_ptr()
            a = np.ascontiguousarray(np.asarray(a).astype(dtype, copy=False))
            keep.append(a)
            return a.ctypes.data

        cols = N.Columns()
        cols.n_vars = len(names)
        cols.inputs_on_device = int(torch_in)
        vals = (C.c_void_p * len(names))(*[per_gate(k, np.float32) for k in names])
        cols.vals = C.cast(vals, C.c_void_p)
        cols.elev = per_gate('elev', np.float32)
        cols.mask = per_gate('mask', np.int8, required=False)
        melt_keys = ('QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG')
        given = any(k in columns for k in melt_keys)
        if given and not all(k in columns for k in melt_keys):
            raise ValueError('simulate_columns: the given melting fields need all of %s' % (melt_keys,))
        if given and not conf['microphysics']['with_melting']:
            raise ValueError('simulate_columns: melting fields given, but the configuration does not melt')
        if given:
            q = np.stack([_host(columns['QmS_v']), _host(columns['QmG_v'])]) if not torch_in else None
            if torch_in:
                import torch
                columns = dict(columns, _q=torch.stack([columns['QmS_v'], columns['QmG_v']]),
                               _fw=torch.stack([columns['fwet_mS'], columns['fwet_mG']]))
            else:
                columns = dict(columns, _q=q, _fw=np.stack([_host(columns['fwet_mS']), _host(columns['fwet_mG'])]))
            cols.q_melt = per_gate('_q', np.float32, (2, n_rays, n_sub, n_gates))
            cols.fw_melt = per_gate('_fw', np.float64, (2, n_rays, n_sub, n_gates))
            cols.has_melting = per_gate('has_melting', np.int8, (n_rays, n_sub), required=False)
        w = columns['quad_weights']
        w = w if _is_torch(w) else np.asarray(w, dtype=np.float64)
        ml = len(tuple(w.shape)) == 3
        want_vis = bool(conf['integration'].get('terrain_visibility', 0))
        if want_vis and ml:
            raise ValueError("integration/terrain_visibility: not defined with the per-gate weights of integration scheme 'ml'")
        if ml:
            cols.wgate = per_gate('quad_weights', np.float64)
            sub_w = np.ones(n_sub)
        else:
            sub_w = np.ascontiguousarray(_host(w), dtype=np.float64)
            if sub_w.shape != (n_sub,):
                if sub_w.shape == (n_rays, n_sub) and (sub_w == sub_w[:1]).all():
                    sub_w = np.ascontiguousarray(sub_w[0])
                else:
                    raise ValueError('simulate_columns: quad_weights must be [n_sub], the same for every radial, '
                                     'or per gate [n_rays, n_sub, n_gates]')
        qp = np.asarray(_host(columns['quad_pts']), dtype=np.float64)
        if not np.isfinite(qp).all():
            raise ValueError('simulate_columns: quad_pts must be finite')
        if qp.shape != (n_rays, n_sub, 2):
            raise ValueError('simulate_columns: quad_pts must be [n_rays, n_sub, 2]')
        az_rad = qp[..., 0] * geo.DEG                  # (the angle of geometry.ray_tables: same sin / cos bits)
        az_sincos = np.ascontiguousarray(np.stack([np.sin(az_rad), np.cos(az_rad)], axis=-1))
        keep += [sub_w, az_sincos]
        cols.az_sincos = az_sincos.ctypes.data
        cols.sub_w = sub_w.ctypes.data

        p = N.SweepParams()
        p.n_rays, p.n_gates, p.n_sub = n_rays, n_gates, n_sub
        p.n_hnodes = p.n_vnodes = n_sub
        p.with_melting = int(conf['microphysics']['with_melting'])
        p.with_attenuation = int(conf['microphysics']['with_attenuation'])
        want_model = self.output_variables in ('all', 'only_model')
        p.integrate_model = int(want_model)
        p.outputs_on_device = 1 if device_outputs is not None else (2 if pinned else 0)
        doppler = conf['doppler']['scheme'] in (1, 2, 3) and conf['radar'].get('type') != 'GPM'
        spectrum = doppler and conf['doppler']['scheme'] == 3
        p.simulate_doppler = int(conf['doppler']['scheme']) if doppler else 0
        vi = {v: i for i, v in enumerate(names)}
        p.var_u, p.var_v, p.var_w = vi['U'], vi['V'], vi['W']
        p.var_rho = vi.get('RHO', -1)
        if spectrum:
            varray = np.ascontiguousarray(self.constants.VARRAY, dtype=np.float64)
            keep.append(varray)
            cols.varray = varray.ctypes.data
            p.n_vbins = len(varray)
            p.c_spectrum = float(self.constants.WAVELENGTH ** 4 / (np.pi ** 5 * conf['radar']['K_squared'] ** 2))
            self._fill_broadening(p, names, float(self.constants.RANGE_RADAR[0]))
        p.geometry_mode = N.GEOM_GROUND_43
        p.terrain_shadow = 0                           # (the caller's masks stand)
        p.range_step = float(conf['radar']['radial_resolution'])
        p.wavelength = float(self.constants.WAVELENGTH)
        p.k_squared = float(conf['radar']['K_squared'])
        p.radial_res = float(conf['radar']['radial_resolution'])
        p.c_zh = float(self.constants.WAVELENGTH ** 4 / (np.pi ** 5 * conf['radar']['K_squared']))
        thr = geo.sensitivity_threshold(conf, self.constants, n_gates) if apply_sensitivity else None
        p.apply_sensitivity = int(thr is not None)
        if thr is not None:
            keep.append(thr)
            cols.sens_thr = thr.ctypes.data
        if doppler and conf['radar']['nyquist_velocity'] is not None:
            # the central sub-radial's angles (doppler_scatter.py:94-96, 436-437)
            c = int(n_sub / 2)
            nyq = np.ascontiguousarray(conf['radar']['nyquist_velocity'](qp[:, c, 1], qp[:, c, 0]), dtype=np.float64)
            keep.append(nyq)
            cols.nyquist = nyq.ctypes.data

        o = N.Outputs()
        res = {}
        if device_outputs is not None:
            for k, ptr in device_outputs.items():
                setattr(o, k, ptr)
        else:
            shape = (n_rays, n_gates)
            spec = [(k, np.float32, shape) for k in RADAR_FIELDS]
            if doppler:
                spec.append(('RVEL', np.float64, shape))
            if spectrum:
                spec.append(('DSPECTRUM', np.float64, shape + (p.n_vbins,)))
            spec.append(('mask', np.float64, shape))
            if want_vis:
                spec.append(('visibility', np.float64, shape))
            if want_model:
                spec.append(('model_vars', np.float64, (len(names),) + shape))
            if pinned:
                views, _, holder = N.carve_block(self._pool, spec, writer=self._lane(lane))
                res = {k: a for (k, _, _), a in zip(spec, views)}
            else:
                res = {k: np.empty(sh, dtype=dt) for k, dt, sh in spec}
            for k, v in res.items():
                setattr(o, k, v.ctypes.data)
        ctx = self._lane(lane)
        if torch_in:
            # the columns are read in place: behind the work queued on torch's current stream, and torch's stream waits
            # for the ingest before it may reuse their memory
            import torch
            ext = torch.cuda.ExternalStream(ctx.stream_ptr(), device=torch.device('cuda', self.device))
            ext.wait_stream(torch.cuda.current_stream(self.device))
        ctx.run_columns(p, cols, o)
        if torch_in:
            torch.cuda.current_stream(self.device).wait_stream(ext)
        if device_outputs is None:
            if pinned:
                holder['ctx'], holder['serial'] = ctx, ctx.submitted
            del keep
            c = int(n_sub / 2)
            for k in ('lats', 'lons', 'dist', 'heights'):
                if k in columns:
                    a = columns[k]
                    res[k] = (a[:, c].cpu().numpy() if _is_torch(a) else np.asarray(a)[:, c]).copy()
        res['n_sub'] = n_sub
        return res

    def get_radar_observables(self, list_subradials):
        """The reference's get_radar_observables (scatter/doppler_scatter.py:49-489) for one radial on the GPU: a list
        of sub-radials -- objects with the attributes of the reference's Radial (values, mask, elev_profile, quad_pt,
        quad_weight, has_melting, lats / lons / dist / heights_profile): this package's, the oracle's or the
        reference's own -- -> one Radial of the observables ZH ... RVEL (no sensitivity cut).  Records that carry
        QmS_v use the given melting fields, the others are melted on the device when the configuration melts.
        Unlike the reference, which folds elev_profile in place, the records are never modified.
        Ragged lists (different gate counts) and weights of different kinds raise ValueError."""
        from .radial import Radial, subradials_to_columns
        subs = list(list_subradials)
        cols = subradials_to_columns(subs, self._column_names(), self.__config['microphysics']['with_melting'])
        n_sub = len(subs)
        res = self.simulate_columns(cols, apply_sensitivity=False)
        c = subs[int(n_sub / 2)]
        values = {k: v[0] for k, v in res.items() if k not in ('mask', 'n_sub', 'lats', 'lons', 'dist', 'heights', 'model_vars')}
        return Radial(values, res['mask'][0], c.lats_profile, c.lons_profile, c.dist_profile, c.heights_profile)

    def _run_rays(self, azimuths, elevations, coords, n_gates, range0, mode, device_outputs=None,
                  apply_sensitivity=True, paths=None, site=None, sub=None, tables=None, lane=0,
                  pinned=False, subbeams=None, members=None, timed=None, product=None):
        """`product`: what is computed on the device behind the sweep and handed back beside it -- or instead of it -- under
        res[product.name]: a product object ("How a product plugs into a sweep call"), built, and its spec checked,
        by the public method.  The plain call pays one test for all of them."""
        if self._model_staged:
            self._sync_edr()
        gates = True                              # the per-gate radar fields travel to the host
        if product is not None:
            for kind, arg in (('members', members), ('timed', timed), ('subbeams', subbeams)):
                if arg is not None and kind in product.refuses:
                    raise ValueError(product.refuses[kind])
            gates = product.gates
        conf = self.__config
        az = np.ascontiguousarray(np.asarray(azimuths, dtype=np.float64).reshape(-1))
        el = np.ascontiguousarray(np.asarray(elevations, dtype=np.float64).reshape(-1))
        if az.shape != el.shape:
            raise ValueError('azimuths and elevations must have the same length')
        n_rays = len(az)
        if sub is None:
            sub = self._cached('sub', lambda: quadrature.subbeams(conf))
        # terrain shadowing and the visibility array (cosmo_pol_amd/shadow.py): every entry point built on this method honours them
        shadow = bool(conf['integration'].get('terrain_shadow', 0))
        want_vis = bool(conf['integration'].get('terrain_visibility', 0)) and subbeams is None
        # (swaths: get_GPM_swath refuses shadowing before it comes here, and so does the library)
        if want_vis and sub.sub_smooth is not None:
            raise ValueError("integration/terrain_visibility: not defined with the per-gate weights of integration scheme 'ml'")
        version = 0
        if tables is not None:
            traj, geo_t = tables
        else:
            version, traj, geo_t = self._ray_tables(az, el, coords, sub)
            if paths is not None or site is not None or not self.reuse_device_tables:
                version = 0

        want_model = self.output_variables in ('all', 'only_model') and members is None and gates
        # a histogram over a model variable: the library integrates the model variables for it, asked for or not
        hg_model = product is not None and product.model_var is not None
        if hg_model:
            if self.output_variables not in ('all', 'only_model') or members is not None:
                raise ValueError("histogram: the ordinate %r needs a call that produces model_vars (output_variables 'all' or "
                                 "'only_model', no ensemble call)" % (('model', product.model_var),))
            if product.model_var not in self._staged_vars:
                raise ValueError('histogram: no staged model variable %r' % (product.model_var,))
        integrate = want_model or hg_model

        def prepare(paths=paths, site=site):
            """The argument structs of cpol_run_sweep for this set of rays (and the arrays they point into)."""
            p = N.SweepParams()
            p.n_rays, p.n_gates, p.n_sub = n_rays, n_gates, sub.n_sub
            p.n_hnodes, p.n_vnodes = len(sub.pts_hor), len(sub.pts_ver)
            p.with_melting = int(conf['microphysics']['with_melting'])
            p.with_attenuation = int(conf['microphysics']['with_attenuation'])
            p.integrate_model = int(integrate)
            p.outputs_on_device = 1 if device_outputs is not None else 2     # host outputs: page-locked, one copy
            # Doppler schemes 1 (analytic mean fall speed), 2 (rcs-weighted) and 3 (the full spectrum); none for GPM
            # (doppler_scatter.py:83-87)
            doppler = (conf['doppler']['scheme'] in (1, 2, 3) and conf['radar'].get('type') != 'GPM'
                       and mode != N.GEOM_SPACEBORNE)
            spectrum = doppler and conf['doppler']['scheme'] == 3
            p.simulate_doppler = int(conf['doppler']['scheme']) if doppler else 0
            vi = {v: i for i, v in enumerate(self._staged_vars)}
            p.var_u, p.var_v, p.var_w = vi['U'], vi['V'], vi['W']
            p.var_rho = vi.get('RHO', -1)
            varray = None
            if spectrum:
                varray = np.ascontiguousarray(self.constants.VARRAY, dtype=np.float64)
                p.n_vbins = len(varray)
                p.c_spectrum = float(self.constants.WAVELENGTH ** 4
                                     / (np.pi ** 5 * conf['radar']['K_squared'] ** 2))
            p.geometry_mode = mode
            p.debug_flags = int(self.debug_flags)
            p.terrain_shadow = int(shadow)
            if site is None:
                re, ke = geo.earth_radius_for_refraction(coords)
                sin_u1, cos_u1, _ = geo.radar_site_constants(coords)
                p.radar_lat, p.radar_lon, p.radar_alt = (float(coords[0]), float(coords[1]),
                                                         float(coords[2]))
                p.ke, p.re = ke, re
                p.sin_u1, p.cos_u1 = sin_u1, cos_u1
            else:
                p.ke, p.re = 1.0, 0.0
            p.range0 = range0
            p.range_step = float(conf['radar']['radial_resolution'])
            p.wavelength = float(self.constants.WAVELENGTH)
            p.k_squared = float(conf['radar']['K_squared'])
            p.radial_res = float(conf['radar']['radial_resolution'])
            p.c_zh = float(self.constants.WAVELENGTH ** 4 / (np.pi ** 5 * conf['radar']['K_squared']))
            if spectrum:
                self._fill_broadening(p, list(self._staged_vars), range0)

            thr = (self._cached(('sens', n_gates),
                                lambda: geo.sensitivity_threshold(conf, self.constants, n_gates))
                   if apply_sensitivity else None)
            p.apply_sensitivity = int(thr is not None)
            t = N.RayTables()
            if paths is not None:
                paths = np.ascontiguousarray(paths, dtype=np.float32)
                if paths.shape != (n_rays, p.n_vnodes, 3, n_gates):
                    raise ValueError('paths must have shape [n_rays, n_vnodes, 3, n_gates] = %s'
                                     % ((n_rays, p.n_vnodes, 3, n_gates),))
            if site is not None:
                site = np.ascontiguousarray(site, dtype=np.float64)
            keep = [traj, geo_t, sub.sub_h, sub.sub_v, sub.sub_w, thr, paths, site]
            t.traj, t.geo = traj.ctypes.data, geo_t.ctypes.data
            t.sub_h, t.sub_v, t.sub_w = sub.sub_h.ctypes.data, sub.sub_v.ctypes.data, sub.sub_w.ctypes.data
            t.sens_thr = thr.ctypes.data if thr is not None else None
            t.site = site.ctypes.data if site is not None else None
            t.paths = paths.ctypes.data if paths is not None else None
            nyq = None
            if doppler and conf['radar']['nyquist_velocity'] is not None:
                # Nyquist velocity of every ray from its nominal elevation / azimuth
                # (doppler_scatter.py:431-437: the central sub-beam's angles)
                nyq = np.ascontiguousarray(conf['radar']['nyquist_velocity'](el, az), dtype=np.float64)
                keep.append(nyq)
            t.nyquist = nyq.ctypes.data if nyq is not None else None
            if varray is not None:
                keep.append(varray)
                t.varray = varray.ctypes.data
            if sub.sub_smooth is not None:        # integration scheme 'ml': per-gate weights
                t.sub_smooth = sub.sub_smooth.ctypes.data
                t.ml_filter = sub.ml_filter.ctypes.data
                t.ml_radius = int(sub.ml_radius)
            t.version = version
            return p, t, keep, doppler, spectrum, varray

        # the structs of an unchanged set of rays are built once (a sweep repeated, the sweeps of a volume scanned
        # again): ~25 us of attribute traffic per call otherwise, half of what a c2 sweep takes on the device
        if version and paths is None and site is None:
            p, t, keep, doppler, spectrum, varray = self._cached(
                ('prepared', version, n_gates, range0, mode, bool(apply_sensitivity), integrate, device_outputs is not None,
                 int(self.debug_flags), self._staged_serial, shadow),
                prepare, lru=16)
        else:
            p, t, keep, doppler, spectrum, varray = prepare()

        if subbeams is not None:
            return self._export_subbeams(p, t, keep, sub, az, el, n_gates, lane, **subbeams)
        if timed is not None:
            # a time-blended sweep (simulate_rays_at): the states it may read, and per ray the earlier state's index in that
            # list and the weight of the one behind it.  (A copy: the prepared structs are shared between calls.)
            tm_states, tm_lo, tm_w = timed
            t = N.RayTables.from_buffer_copy(t)
            t.time_blend = 1
            t.ray_state, t.ray_weight = tm_lo.ctypes.data, tm_w.ctypes.data
            keep = list(keep) + [tm_lo, tm_w]
        o = N.Outputs()
        res = {}
        geom = part = None
        held = ()                                 # the holders of blocks that the device reads in place during this call
        if product is not None:
            held = []

            def take(spec):
                """A clean block (no writer is named) for arrays of the product that the host writes now."""
                views, addresses, holder = N.carve_block(self._pool, spec)
                held.append(holder)
                return views, addresses
            structs, alive = product.attach(N, az, n_gates, len(members) if members is not None else None, doppler, spectrum,
                                            self._staged_vars, take if device_outputs is None else None)
            for slot, struct in structs.items():
                setattr(o, slot, C.pointer(struct))
            keep = list(keep) + alive
        if device_outputs is not None:
            for k, ptr in device_outputs.items():
                # an array of the sweep itself (one look-up, however many products there are); a dict is some product's entry
                # (`species` is listed in no table: its key is its product's name)
                if k not in _PRODUCT_OUTPUTS and not isinstance(ptr, dict):
                    setattr(o, k, ptr)
                elif product is None or product.name != k:
                    raise ValueError('device_outputs[%r] without %s' % (k, _PRODUCT_OUTPUTS.get(k, 'its product (%s=)' % k)))
                else:
                    product.bind_device(ptr)
        else:
            shape = (n_rays, n_gates)
            gshape = shape                        # (gate coordinates: once, whatever the number of members)
            if members is not None:               # an ensemble call: a leading member axis on every radar field
                shape = (len(members),) + shape
            spec = [(k, np.float32, shape) for k in RADAR_FIELDS] if gates else []
            if doppler and gates:
                spec.append(('RVEL', np.float64, shape))
            if spectrum and gates and (product is None or product.spectrum):
                spec.append(('DSPECTRUM', np.float64, shape + (len(varray),)))
            # (pinned calls only: a blocking call would have to widen the bytes on the caller's thread at once -- ~1 ns per gate,
            # more than the 7 bytes per gate cost on PCIe; measured on the c5 swaths, 1.7 M gates: 8.5 -> 12.7 ms per step)
            mask8 = self.compact_mask and pinned and 2 * sub.n_sub <= 127
            if gates:
                spec.append(('mask_sum8', np.int8, shape) if mask8 else ('mask', np.float64, shape))
            # gate coordinates of the central sub-beam depend on the ray tables only: of an
            # unchanged table set (version tag) they are copied from the device once
            gkey = ('geom', version, n_gates) if version else None
            geom = self._cache.get(gkey) if gkey else None
            if geom is None:
                spec += [('lats', np.float64, gshape), ('lons', np.float64, gshape),
                         ('dist', np.float32, gshape), ('heights', np.float32, gshape)]
            if want_vis and gates:
                spec.append(('visibility', np.float64, gshape))
            if want_model:
                spec.append(('model_vars', np.float64, (len(self._staged_vars),) + shape))
            # every host output is a view of ONE block of page-locked memory from the operator's pool (N.carve_block); the
            # product's arrays lie behind the sweep's own in the same block: they ride the one copy
            extra = product.arrays() if product is not None else []
            views, addresses, holder = N.carve_block(self._pool, spec + extra, writer=self._lane(lane))
            for (k, _, _), a, address in zip(spec, views, addresses):
                res[k] = a
                setattr(o, k, address)
            if extra:
                part = {}
                for (k, _, _), a, address in zip(extra, views[len(spec):], addresses[len(spec):]):
                    part[k] = a
                    product.bind(k, address)
            del views
        ctx = self._lane(lane)
        if members is not None:
            ctx.run_sweep_members(p, t, members, o)
        elif timed is not None:
            ctx.run_sweep_members(p, t, tm_states, o)
        else:
            ctx.run_sweep(p, t, o)
        for h in held:                            # (the device reads such a block until this call is done)
            h['ctx'], h['serial'] = ctx, ctx.submitted
        del keep
        if device_outputs is None and 'mask_sum8' in res:
            # `mask` is made from its one-byte form when it is first read (after wait(lane) for a pinned call, like every
            # other array of the result)
            lazy = LazyDict()
            for k, v in res.items():
                lazy[k] = v
            lazy.add('mask', _mask_from_sum(res['mask_sum8'], sub.n_sub))
            res = lazy
        if device_outputs is None:
            if pinned:
                holder['ctx'], holder['serial'] = ctx, ctx.submitted    # a copy into the block is in flight until wait(lane)
            else:
                ctx.synchronize()                       # blocking call: results complete, IndexError raised here
            if geom is None and gkey is not None:
                if pinned:
                    ctx.synchronize()                   # once per table set: the arrays are complete
                # (own read-only copies: shared by every later result of this table set)
                made = {k: res[k].copy() for k in _COORDS}
                for a in made.values():
                    a.flags.writeable = False
                geom = self._cached(gkey, lambda: made, lru=32)
            if geom is not None:
                res.update(geom)
            if part is not None:
                def coords(key, make):
                    """Coordinate arrays of the product's own, made of the gate coordinates by make(those)."""
                    if geom is None:              # (no table version: this call's own coordinate arrays)
                        if pinned:
                            ctx.synchronize()
                        return make(res)

                    def frozen():
                        # (read-only, like the gate coordinates they are made of: shared by every later result of this table set)
                        made = make(geom)
                        for a in made.values():
                            a.flags.writeable = False
                        return made
                    return self._cached((product.name + '_geom', gkey) + key, frozen, lru=16)
                res[product.name] = product.finish(part, coords)
        res['n_sub'] = sub.n_sub
        return res

    def _cached(self, key, make, lru=None):
        with self._lock:
            return self._cached_locked(key, make, lru)

    def _cached_locked(self, key, make, lru=None):
        c = self._cache
        if key in c:
            return c[key]
        if lru is not None:
            old = [k for k in c if k[:1] == key[:1]]
            for k in old[:max(0, len(old) - lru + 1)]:
                del c[k]
        c[key] = make()
        return c[key]

    # ------------------------------------------------------------------ ensembles
    # (replaces in the reference: nothing -- it runs one model state per process)
    @property
    def n_members(self):
        """Model states staged on the device: 0 without a model, 1 after load_model_*, M after load_model_ensemble."""
        return self._n_members if self._model_staged else 0

    def _member_input(self, i, m, zlevels, proj_info, resolution, cfilename):
        from . import model_io
        if isinstance(m, (str, bytes, os.PathLike)):
            want_n = self.__config['refraction']['scheme'] == 2 and i == 0
            f = model_io.read_model_file(m, cfilename, want_refractivity=want_n, want_edr=self._wants_edr(),
                                         grib_table=self.grib_table)
            return {'data': f['data'], 'zlevels': f['zlevels'], 'proj_info': f['proj_info'],
                    'resolution': f['resolution'], 'time': f.get('time')}
        if zlevels is None or proj_info is None or resolution is None:
            raise ValueError('ensemble member %d is a dict of arrays: zlevels, proj_info and resolution are needed' % i)
        return {'data': m, 'zlevels': zlevels, 'proj_info': proj_info, 'resolution': resolution, 'time': None}

    def load_model_ensemble(self, members, zlevels=None, proj_info=None, resolution=None, cfilename=None):
        """Loads M >= 2 states of ONE model -- ensemble members, or a series of forecast times -- under the operator's one set of
        scattering and integral tables.  Each member is a file name (anything load_model_file reads; decoded on the host)
        or a `data` dict as for load_model_arrays (then zlevels, proj_info and resolution are given once, for all).  Every
        member must have the same variables, shape, grid and z-levels; ValueError names the member and what differs, and
        leaves the operator as it was.  Member 0 becomes "the model": every existing call behaves exactly as after
        load_model_arrays(member 0); select_member / the *_ensemble calls reach the others.  Device memory per further
        member: the cube alone (n_vars x nz x ny x nx x 4 bytes).  Any later load_model_* or restaging of the cube (a
        configuration that changes the variable set) drops the members again."""
        if self.distributed:
            raise NotImplementedError('ensembles with a process group: sharding members or rays over ranks is not built')
        members = list(members)
        from . import ensemble
        ins = [self._member_input(i, m, zlevels, proj_info, resolution, cfilename) for i, m in enumerate(members)]
        ensemble.check_members(ins)
        m0 = ins[0]
        self.load_model_arrays(m0['data'], m0['zlevels'], m0['proj_info'], m0['resolution'], time=m0['time'])
        names = self._staged_vars
        for i, m in enumerate(ins[1:], start=1):
            missing = [k for k in names if k not in m['data']]
            if missing:
                raise ValueError('ensemble member %d: missing %s' % (i, missing))
            self._ctx.stage_member(i, [m['data'][k] for k in names])
        self._n_members = len(ins)
        self._member_times = [m['time'] for m in ins]

    def select_member(self, m):
        """Every later ordinary call (simulate_rays, get_PPI, interpolate_rays, submit_volume ...) on every lane reads member
        `m`: a pointer swap on the device, no copy.  Host-side views (`dic_vars`, the refractivity N of refraction scheme 2)
        stay member 0's."""
        m = int(m)
        if not 0 <= m < self.n_members:
            raise ValueError('select_member(%d): %d member(s) staged' % (m, self.n_members))
        with self._lock:
            for c in [self._ctx] + list(self._lane_ctx):
                c.select_member(m)
            self._member = m

    def _members_arg(self, members):
        if self.distributed:
            raise NotImplementedError('ensembles with a process group: sharding members or rays over ranks is not built')
        if self.output_variables != 'only_radar':
            raise NotImplementedError("ensemble calls do not return antenna-integrated model variables "
                                      "(use output_variables='only_radar')")
        if not self._check_ready():
            raise ValueError('no model loaded')
        members = list(range(self.n_members)) if members is None else [int(m) for m in members]
        if not members:
            raise ValueError('members: empty list')
        for m in members:
            if not 0 <= m < self.n_members:
                raise ValueError('member %d: %d member(s) staged' % (m, self.n_members))
        if len(set(members)) != len(members):
            raise ValueError('members: %r lists a member twice' % (members,))
        return members

    def simulate_rays_ensemble(self, azimuths, elevations, members=None, on_device=False, device_outputs=None,
                               apply_sensitivity=True, lane=0, form=None, pinned=False, superob=None, keep_gates=False,
                               rays_per_block=0):
        """simulate_rays for several members of the ensemble at once: the dict of simulate_rays with a leading member axis
        (in the order of `members`; None = all) on the radar fields, `mask` included, and the gate coordinates once.
        form='shared': cpol_run_sweep_members -- geometry once per sub-beam gate, then the members; the member list is cut
        into chunks whose work buffers (cpol_mem_info's per_gate x sub-beam gates x members) fit
        `sequence_memory_budget`.  form='per_member': select_member + the ordinary sweep, member by member (keeps the fused
        single-beam kernels).  form=None: 'shared' from `ensemble_shared_from` sub-beams per radial.  Either way every
        member's arrays carry the bits of simulate_rays on an operator loaded with that member alone.
        `device_outputs`: {field: device pointer} of [n_members, n_rays, n_gates] arrays (geometry: [n_rays, n_gates]).
        `pinned`: as for simulate_rays when the members fit one chunk; with several chunks the call waits.
        `superob`, `keep_gates`, `rays_per_block`: as for simulate_rays_superob; the arrays of res['superob'] gain the member axis (the
        window coordinates come once).  A window never holds gates of two members."""
        return self._ensemble_rays(azimuths, elevations, members, device_outputs, apply_sensitivity, lane, form, pinned,
                                   None if superob is None else SO.Windows(superob, keep_gates, rays_per_block, self.distributed))

    def simulate_rays_ensemble_stats(self, azimuths, elevations, stats, members=None, keep_members=False, form=None, lane=0,
                                     pinned=False, device_outputs=None, apply_sensitivity=True):
        """simulate_rays_ensemble handing back ENSEMBLE STATISTICS instead of the members: `stats` is an
        ensemble_stats.EnsembleStats, and the result is the gate coordinates once and res['stats'] = {'mean', 'spread', 'min',
        'max': {field: [n_rays, n_gates]} (those `stats` asks for), 'count': {field: uint16}, 'exceed': {field: uint16 [n_thr,
        n_rays, n_gates]}, 'n_members': M} -- folded on the device behind the sweeps' kernels, member after member in the order
        of `members` (ensemble_stats.fold / finish state the rule; the device result carries the bits of
        ensemble_stats.reduce(simulate_rays_ensemble(...), stats)).  An ensemble_stats.EnsembleQuantiles adds 'quantile': {field:
        [n_q, n_rays, n_gates]} (medians, percentiles; at most 128 members, ValueError beyond).  Without `keep_members` no per-member array is produced for
        the host or copied; with it everything simulate_rays_ensemble returns comes back beside the statistics.
        `form`, `members`, `lane`, `apply_sensitivity`: as for simulate_rays_ensemble; whatever the form and however
        `sequence_memory_budget` cuts the member list, the first call of the pass begins it, the last finishes it, all go to
        the one lane, and the bits are the same.  `pinned`: do not wait (call wait(lane)); with several calls it waits.
        `device_outputs`: {'stats': {'mean' | 'spread' | 'min' | 'max' | 'exceed' | 'quantile': {field: device pointer}, 'count': device
        pointer of [10, n_rays, n_gates]}} (and, with keep_members, the per-member pointers of simulate_rays_ensemble).
        An ensemble_verify.EnsembleVerification needs observations: simulate_rays_ensemble_verify takes it (ValueError here).
        NotImplementedError where simulate_rays_ensemble raises it: a process group, spaceborne geometry, refraction scheme 2."""
        if not isinstance(stats, ES.EnsembleStats):
            raise ValueError('stats: a cosmo_pol_amd.ensemble_stats.EnsembleStats, got %r' % (stats,))
        if isinstance(stats, EV.EnsembleVerification):
            raise ValueError('an EnsembleVerification needs observations: simulate_rays_ensemble_verify(azimuths, elevations, stats, '
                             'observations, ...) takes it')
        members = None if members is None else list(members)
        return self._ensemble_rays(azimuths, elevations, members, device_outputs, apply_sensitivity, lane, form, pinned,
                                   ES.Fold(stats, keep_members, capacity=self.n_members if members is None else len(members)))

    def simulate_rays_ensemble_verify(self, azimuths, elevations, stats, observations=None, members=None, keep_members=False, form=None,
                                      lane=0, pinned=False, device_outputs=None, apply_sensitivity=True):
        """simulate_rays_ensemble_stats with a VERIFICATION of the ensemble against an observed sweep: `stats` is an
        ensemble_verify.EnsembleVerification, `observations` {field: [n_rays, n_gates]} holds a NumPy array of the field's type for
        every verified field (linear units, NaN = no observation), and res['stats'] gains 'verify': {'below' | 'equal': {field:
        uint16 [n_rays, n_gates]}, 'crps': {field: [n_rays, n_gates]}} -- the rank of the observation among the members and the CRPS
        per gate, formed on the device behind the statistics (k_member_verify; ensemble_verify states the rule, and the device
        result carries the bits of ensemble_verify.reduce(simulate_rays_ensemble(...), observations, stats)).  At most 128 members.
        `fields` and `fair` go with every call of the pass, the observations with the last.  The other keywords are those of
        simulate_rays_ensemble_stats.  With `device_outputs` the observations are device pointers, device_outputs['stats']['obs'] =
        {field: pointer} (`observations` stays None), and 'below' | 'equal' | 'crps': {field: pointer} take the scores.
        ValueError for observations of a wrong shape or dtype, a verified field without one, more than 128 members."""
        if not isinstance(stats, EV.EnsembleVerification):
            raise ValueError('stats: a cosmo_pol_amd.ensemble_verify.EnsembleVerification, got %r' % (stats,))
        dev_obs = (device_outputs or {}).get('stats', {}).get('obs')
        if (observations is None) == (dev_obs is None):
            raise ValueError("an EnsembleVerification needs observations (NumPy arrays), or with device_outputs the device "
                             "pointers device_outputs['stats']['obs'], and not both")
        if dev_obs is not None:
            for k in stats.verify:
                if k not in dev_obs:
                    raise ValueError("device_outputs['stats']['obs']: no observations for the verified field %r" % (k,))
        else:
            if device_outputs is not None:
                raise ValueError("with device_outputs the observations are device pointers under device_outputs['stats']['obs']")
            n_rays = len(np.asarray(azimuths).reshape(-1))
            observations = EV.check_observations(stats, stats.verify, observations, (n_rays, len(self.constants.RANGE_RADAR)))
        members = None if members is None else list(members)
        return self._ensemble_rays(azimuths, elevations, members, device_outputs, apply_sensitivity, lane, form, pinned,
                                   ES.Fold(stats, keep_members, capacity=self.n_members if members is None else len(members),
                                           observations=observations))

    def _ensemble_rays(self, azimuths, elevations, members, device_outputs, apply_sensitivity, lane, form, pinned, product=None):
        members = self._members_arg(members)
        conf = self.__config
        coords = self._ensemble_coords()
        from . import ensemble
        sub = self._cached('sub', lambda: quadrature.subbeams(conf))
        if form is None:
            form = ensemble.choose_form(sub.n_sub, self.ensemble_shared_from)
        if form not in ('shared', 'per_member'):
            raise ValueError("form must be 'shared', 'per_member' or None")
        rr = self.constants.RANGE_RADAR
        n_rays = len(np.asarray(azimuths).reshape(-1))
        ctx = self._lane(lane)
        if form == 'shared':
            chunks = self._shared_member_chunks(ctx, members, sub.n_sub * len(rr) * n_rays)
        else:
            chunks = [[m] for m in members]
        # a product over the members: the chunks are ONE pass, and only its last call holds the result; any other comes per member
        fold = product is not None and product.over_members
        if product is not None and not fold and device_outputs is not None and len(chunks) > 1:
            raise ValueError('simulate_rays_ensemble: superobservations into device outputs need the members in one chunk')
        parts, done = [], 0
        try:
            for i, chunk in enumerate(chunks):
                if fold:
                    # the pass: begun by the first call, finished by the last, every call on this lane
                    product.phase = (1 if i == 0 else 0) | (2 if i == len(chunks) - 1 else 0)
                dev = None
                if device_outputs is not None:
                    dev = self._offset_outputs(device_outputs, done, n_rays, len(rr))
                if form == 'per_member':
                    ctx.select_member(chunk[0])
                    r = self._run_rays(azimuths, elevations, coords, len(rr), float(rr[0]), N.GEOM_GROUND_43, device_outputs=dev,
                                       apply_sensitivity=apply_sensitivity, lane=lane, pinned=pinned, product=product)
                else:
                    r = self._run_rays(azimuths, elevations, coords, len(rr), float(rr[0]), N.GEOM_GROUND_43, device_outputs=dev,
                                       apply_sensitivity=apply_sensitivity, lane=lane, pinned=pinned and len(chunks) == 1,
                                       members=chunk, product=product)
                parts.append(r)
                done += len(chunk)
        finally:
            if form == 'per_member':
                ctx.select_member(self._member)
        if device_outputs is not None:
            return parts[-1]
        if form == 'shared' and len(parts) == 1:
            return parts[0]
        once = _ONCE + ('n_sub',)
        join = np.stack if form == 'per_member' else np.concatenate
        if fold and not product.gates:
            # (no per-member array came: the coordinates of the first call, the result of the last)
            if pinned and len(parts) > 1:
                self.wait(lane)
            out = {k: v for k, v in parts[0].items() if k in once}
        else:
            if pinned:
                self.wait(lane)                    # (the members are joined on the host: their copies must have landed)
            out = {k: (parts[0][k] if k in once else join([p[k] for p in parts])) for k in parts[0].keys()
                   if product is None or k != product.name}
        if product is not None:
            out[product.name] = product.join([p.get(product.name) for p in parts], join)
        return out

    def _ensemble_coords(self):
        """The radar's coordinates for an ensemble call; NotImplementedError for the geometries such a call does not take."""
        conf = self.__config
        coords = conf['radar']['coords']
        if coords[2] > K.MAX_MODEL_HEIGHT:
            raise NotImplementedError('spaceborne geometry: use get_GPM_swath')
        if conf['refraction']['scheme'] == 2:
            raise NotImplementedError('ensemble calls use the 4/3-earth ray paths (refraction scheme 1)')
        return coords

    def _shared_member_chunks(self, ctx, members, sub_gates):
        """The member list of a 'shared' call cut into chunks whose work buffers (cpol_mem_info's per_gate x `sub_gates`
        sub-beam gates x members) fit `sequence_memory_budget` (None: a third of the free device memory)."""
        from . import ensemble
        free, _, per_gate = ctx.mem_info()
        budget = self.sequence_memory_budget if self.sequence_memory_budget is not None else free // 3
        return ensemble.plan_member_chunks(members, per_gate * sub_gates, budget)

    def _offset_outputs(self, device_outputs, n_before, n_rays, n_gates):
        """The caller's device pointers moved behind the `n_before` members already written (gate coordinates: not moved)."""
        n_vb = len(self.constants.VARRAY) if self.__config['doppler']['scheme'] == 3 else 0
        width = {'RVEL': 8, 'mask': 8, 'DSPECTRUM': 8 * n_vb, 'sz_total': 4 * N.N_SZ, 'mask_sum8': 1}
        out = {}
        for k, ptr in device_outputs.items():
            if k in _ONCE + ('superob', 'stats'):
                out[k] = ptr
            else:
                out[k] = int(ptr) + n_before * n_rays * n_gates * width.get(k, 4)
        return out

    def _ensemble_scans(self, scan_type, members, sweeps, elevations, azimuths):
        members = self._members_arg(members)
        per = [[] for _ in members]
        for az, el in sweeps:
            res = self.simulate_rays_ensemble(az, el, members=members)
            for j in range(len(members)):
                one = {k: (v[j] if isinstance(v, np.ndarray) and k not in _ONCE else v)
                       for k, v in res.items()}
                per[j].append(self._package(one, az, el))
        pos = self.get_pos_and_time()
        times = getattr(self, '_member_times', None) or [None] * self.n_members
        out = []
        for j, m in enumerate(members):
            pt = dict(pos)
            if times[m] is not None:
                pt['time'] = times[m]
            out.append(self._finish_scan(RadarScan(scan_type, list(elevations), list(azimuths), self.constants.RANGE_RADAR,
                                                   pt, per[j])))
        return out

    def get_PPI_ensemble(self, elevations, azimuths=None, az_step=None, az_start=0, az_stop=359, members=None):
        """get_PPI for the members of the ensemble: a list of RadarScan, one per member of `members` (None = all), each what
        get_PPI gives on an operator loaded with that member alone (sensitivity cut and packaging as there)."""
        if np.isscalar(elevations):
            elevations = [elevations]
        if az_step is None:
            az_step = self.__config['radar']['3dB_beamwidth']
        if azimuths is None or np.any(np.equal(azimuths, None)):
            if az_start > az_stop:
                azimuths = np.hstack((np.arange(az_start, 360., az_step), np.arange(0, az_stop + az_step, az_step)))
            else:
                azimuths = np.arange(az_start, az_stop + az_step, az_step)
        azimuths = np.asarray(azimuths, dtype=float)
        sweeps = [(azimuths, np.full(len(azimuths), float(e))) for e in elevations]
        return self._ensemble_scans('ppi', members, sweeps, elevations, azimuths)

    def get_RHI_ensemble(self, azimuths, elevations=None, elev_step=None, elev_start=0, elev_stop=90, members=None):
        """get_RHI for the members of the ensemble: a list of RadarScan, one per member (see get_PPI_ensemble)."""
        if np.isscalar(azimuths):
            azimuths = [azimuths]
        if elevations is None or np.any(np.equal(elevations, None)):
            if elev_step is None:
                elev_step = self.__config['radar']['3dB_beamwidth']
            elevations = np.arange(elev_start, elev_stop + elev_step, elev_step)
        elevations = np.asarray(elevations, dtype=float)
        sweeps = [(np.full(len(elevations), float(a)), elevations) for a in azimuths]
        return self._ensemble_scans('rhi', members, sweeps, elevations, azimuths)

    # ------------------------------------------------------------------ time-interpolated scans
    # (replaces in the reference: nothing -- it simulates every ray at the time of the one model state it read)
    def load_model_series(self, states, times=None, zlevels=None, proj_info=None, resolution=None, cfilename=None):
        """load_model_ensemble for a series of forecast times, plus the times: `states` as its `members`, `times` one per
        state -- numbers (seconds on one clock) or datetimes, strictly increasing; None takes each file's own time
        (ValueError if a state has none).  State 0 becomes "the model"; the *_at calls simulate rays at any time inside
        the series.  Whatever drops the members (a later load_model_*, a restaged cube) drops the series too."""
        from . import timeline
        states = list(states)
        if times is not None and len(list(times)) != len(states):
            raise ValueError('load_model_series: %d times for %d states' % (len(list(times)), len(states)))
        if times is not None:
            secs = timeline.check_series(timeline.as_seconds(list(times)))      # (before anything is staged)
        self.load_model_ensemble(states, zlevels=zlevels, proj_info=proj_info, resolution=resolution, cfilename=cfilename)
        if times is None:
            own = list(self._member_times)
            for i, t in enumerate(own):
                if t is None:
                    raise ValueError('load_model_series: state %d carries no time of its own; give `times`' % i)
            secs = timeline.check_series(timeline.as_seconds(own))
        self._series = (self._staged_serial, len(states), secs)

    @property
    def series_times(self):
        """float64 seconds of the staged series (read-only), or None when no series is staged."""
        sr = getattr(self, '_series', None)
        if sr is None or not self._model_staged or sr[0] != self._staged_serial or sr[1] != self._n_members:
            return None
        out = sr[2].view()
        out.flags.writeable = False
        return out

    def _timed_check(self):
        if self.distributed:
            raise NotImplementedError('time-interpolated scans with a process group: sharding rays over ranks is not built')
        conf = self.__config
        if conf['radar']['coords'][2] > K.MAX_MODEL_HEIGHT:
            raise NotImplementedError('spaceborne geometry: time-interpolated scans take ground radars')
        if conf['refraction']['scheme'] == 2:
            raise NotImplementedError('time-interpolated scans use the 4/3-earth ray paths (refraction scheme 1): with '
                                      'scheme 2 the ray path would depend on the time')
        if not self._check_ready():
            raise ValueError('no model loaded')
        if self.series_times is None:
            raise ValueError('no series staged (load_model_series)')

    def simulate_rays_at(self, azimuths, elevations, times, on_device=False, device_outputs=None, apply_sensitivity=True,
                         lane=0, pinned=False):
        """simulate_rays with the model at the time of every ray: `times` is one value (number or datetime, on the clock
        of load_model_series) or one per ray, inside the series -- ValueError otherwise, no extrapolation.  A ray between
        two states reads both, blended per staged variable by timeline.blend_states' rule on the device (k_interp_timed);
        a ray on a state's time reads that state alone.  The dict of simulate_rays (model variables with
        output_variables='all'), every array with the bits of simulate_rays on an operator loaded with the host-blended
        cube.  Only the states the rays need are listed for the library; rays that need more than 64 are cut into
        consecutive groups (host outputs only; with several groups a pinned call waits)."""
        return self._simulate_rays_at(azimuths, elevations, times, device_outputs=device_outputs,
                                      apply_sensitivity=apply_sensitivity, lane=lane, pinned=pinned)

    def simulate_rays_at_superob(self, azimuths, elevations, times, superob, keep_gates=False, rays_per_block=0,
                                 device_outputs=None, apply_sensitivity=True, lane=0, pinned=False):
        """simulate_rays_at handing back superobservations: `superob`, `keep_gates`, `rays_per_block` as for
        simulate_rays_superob (ValueError when the rays fall into several groups of states: a window would cross them)."""
        return self._simulate_rays_at(azimuths, elevations, times, device_outputs=device_outputs,
                                      apply_sensitivity=apply_sensitivity, lane=lane, pinned=pinned,
                                      product=SO.Windows(superob, keep_gates, rays_per_block, self.distributed))

    def _simulate_rays_at(self, azimuths, elevations, times, device_outputs=None, apply_sensitivity=True, lane=0, pinned=False,
                          product=None, radar=None, source=0):
        self._timed_check()
        from . import timeline
        az = np.asarray(azimuths, dtype=np.float64).reshape(-1)
        el = np.asarray(elevations, dtype=np.float64).reshape(-1)
        if az.shape != el.shape:
            raise ValueError('azimuths and elevations must have the same length')
        tt = timeline.as_seconds(times)
        if tt.ndim == 0 or tt.size == 1:
            tt = np.full(len(az), float(tt.reshape(-1)[0]))
        tt = tt.reshape(-1)
        if len(tt) != len(az):
            raise ValueError('times: one value, or one per ray (%d rays, %d times)' % (len(az), len(tt)))
        lo, w = timeline.bracket(self.series_times, tt)
        groups = timeline.plan_ray_groups(lo, w, N.MEMBERS_PER_CALL)
        if len(groups) > 1 and device_outputs is not None:
            raise ValueError('simulate_rays_at: the rays read more than %d states; with device outputs split the rays'
                             % N.MEMBERS_PER_CALL)
        if len(groups) > 1 and product is not None:     # (a window, or a block of a pass, would cross the groups)
            raise ValueError('simulate_rays_at: the rays read more than %d states; %s' % (N.MEMBERS_PER_CALL, product.refuses['groups']))
        coords = self.__config['radar']['coords'] if radar is None else self._radar_arg(radar)
        rr = self.constants.RANGE_RADAR
        if product is not None and hasattr(product, 'set_plane'):     # (one group: refused above otherwise)
            self._set_plane(product, az, el, coords, None, source, device_outputs, lane)
        parts = []
        for r0, r1, first, count in groups:
            tm = (np.arange(first, first + count, dtype=np.int32), np.ascontiguousarray(lo[r0:r1] - first, dtype=np.int32),
                  np.ascontiguousarray(w[r0:r1], dtype=np.float32))
            parts.append(self._run_rays(az[r0:r1], el[r0:r1], coords, len(rr), float(rr[0]), N.GEOM_GROUND_43,
                                        device_outputs=device_outputs, apply_sensitivity=apply_sensitivity, lane=lane,
                                        pinned=pinned and len(groups) == 1, timed=tm, product=product))
        if len(parts) == 1:
            return parts[0]
        return {k: (v if not isinstance(v, np.ndarray) else
                    np.concatenate([q[k] for q in parts], axis=1 if k == 'model_vars' else 0))
                for k, v in parts[0].items()}

    def _scan_at(self, scan_type, sweeps, times, elevations, azimuths):
        self._timed_check()
        from . import timeline
        times = [times] if np.isscalar(times) or isinstance(times, (datetime.datetime, np.datetime64)) else list(times)
        if len(times) != len(sweeps):
            raise ValueError('times: one value or one array per sweep (%d sweeps, %d entries)' % (len(sweeps), len(times)))
        full = []
        for (az, el), t in zip(sweeps, times):
            t = timeline.as_seconds(t)
            full.append((az, el, np.full(len(az), float(t)) if t.ndim == 0 else t.reshape(-1)))
        out = []
        for group in self._sweep_groups(full):                # (the memory-budget rule of the ordinary scans)
            res = self.simulate_rays_at(np.concatenate([g[0] for g in group]), np.concatenate([g[1] for g in group]),
                                        np.concatenate([g[2] for g in group]))
            r0 = 0
            for az, el, _ in group:
                r1 = r0 + len(az)
                part = {k: (v[:, r0:r1] if k in ('model_vars',) else v[r0:r1]) if isinstance(v, np.ndarray) else v
                        for k, v in res.items()}
                out.append(self._package(part, az, el))
                r0 = r1
        return self._finish_scan(RadarScan(scan_type, list(elevations), list(azimuths), self.constants.RANGE_RADAR,
                                           self.get_pos_and_time(), out))

    def get_PPI_at(self, elevations, times, azimuths=None, az_step=None, az_start=0, az_stop=359):
        """get_PPI with the model at the time of every sweep or ray: `times` holds one value per sweep, or one array (a time
        per ray) per sweep.  The RadarScan get_PPI returns; every sweep equals simulate_rays_at of its rays."""
        if np.isscalar(elevations):
            elevations = [elevations]
        if az_step is None:
            az_step = self.__config['radar']['3dB_beamwidth']
        if azimuths is None or np.any(np.equal(azimuths, None)):
            if az_start > az_stop:
                azimuths = np.hstack((np.arange(az_start, 360., az_step), np.arange(0, az_stop + az_step, az_step)))
            else:
                azimuths = np.arange(az_start, az_stop + az_step, az_step)
        azimuths = np.asarray(azimuths, dtype=float)
        sweeps = [(azimuths, np.full(len(azimuths), float(e))) for e in elevations]
        return self._scan_at('ppi', sweeps, times, elevations, azimuths)

    def get_RHI_at(self, azimuths, times, elevations=None, elev_step=None, elev_start=0, elev_stop=90):
        """get_RHI with the model at the time of every sweep or ray (see get_PPI_at)."""
        if np.isscalar(azimuths):
            azimuths = [azimuths]
        if elevations is None or np.any(np.equal(elevations, None)):
            if elev_step is None:
                elev_step = self.__config['radar']['3dB_beamwidth']
            elevations = np.arange(elev_start, elev_stop + elev_step, elev_step)
        elevations = np.asarray(elevations, dtype=float)
        sweeps = [(np.full(len(elevations), float(a)), elevations) for a in azimuths]
        return self._scan_at('rhi', sweeps, times, elevations, azimuths)

    def _simulate_sweeps(self, sweeps):
        """[(az, el), ...] -> packaged sweeps.  The reference runs the sweeps of a scan one
        after the other (radar_operator.py:429-432); here up to `lanes` of them are in
        flight together, one host thread per lane (the library calls release the GIL)."""
        if self.distributed:
            res = self._simulate_volume_sharded(sweeps)
            if res is None:
                return None                   # gather_to: this rank computed its share, another holds the scan
            return [self._package(r, az, el) for r, (az, el) in zip(res, sweeps)]
        if self.pipeline_single_beam_scans and len(sweeps) > 1 and self.lanes > 1 \
                and self._cached('sub', lambda: quadrature.subbeams(self.__config)).n_sub == 1:
            # Single-beam scans are bound by PCIe, not by their kernels (a 360 x 500 sweep: 0.15 ms on the device, 0.17 ms for its
            # 9.4 MB of results): every sweep is queued on a lane with page-locked outputs and the call waits once, at the end --
            # the copy of one sweep runs beside the kernels of the next (a 5-elevation volume with melting layer: 0.93 ms against
            # 1.37 ms as ONE launch sequence, whose one copy overlaps nothing; bench.py's c3 step / `api_ms`).  Same bits
            # (tests/test_gpu_headline.py::test_c3_step_vs_oracle_and_blocking_path).
            res = self._over_lanes(sweeps, lambda az, el, lane: self.simulate_rays(az, el, pinned=True, lane=lane))
            return [self._package(r, az, el) for r, (az, el) in zip(res, sweeps)]
        if self.volume_in_one_sequence and len(sweeps) > 1:
            # all sweeps of the scan as ONE launch sequence (rays of different elevations / azimuths in one
            # cpol_run_sweep call): one submission, 7-12 kernel launches and one device-to-host copy per
            # volume instead of per sweep; the per-sweep results are row slices of the volume's arrays --
            # bit-identical to the sweeps run one by one (tests/test_gpu_fullsize.py).  The work buffers of a
            # sequence grow with its sub-beam gates (a 5-elevation volume with 49 sub-beams: 53 GB), so a scan
            # is cut into groups of whole sweeps that fit `sequence_memory_budget`, and a group the device
            # still has no room for is run sweep by sweep.
            out = []
            for group in self._sweep_groups(sweeps):
                try:
                    out.extend(self._simulate_group(group))
                except MemoryError:
                    if len(group) == 1:
                        raise
                    out.extend(r for sw in group for r in self._simulate_group([sw]))
            return out
        n_par = min(self.lanes, len(sweeps))
        if n_par <= 1:
            return [self._package(self._simulate_sweep(az, el), az, el) for az, el in sweeps]
        import queue
        from concurrent.futures import ThreadPoolExecutor
        free = queue.Queue()
        for i in range(n_par):
            self._lane(i)
            free.put(i)

        def one(sw):
            lane = free.get()
            try:
                return self._package(self._simulate_sweep(sw[0], sw[1], lane=lane), sw[0], sw[1])
            finally:
                free.put(lane)
        with ThreadPoolExecutor(max_workers=n_par) as pool:
            return list(pool.map(one, sweeps))

    def _over_lanes(self, sweeps, call, n_par=None):
        """[call(az, el, lane) per sweep]: one pinned call per sweep, queued over `n_par` lanes (None: all the operator has),
        and one wait per lane at the end.  Every lane is drained whatever happened; the first failure is re-raised."""
        if not self._check_ready():
            raise ValueError('no model loaded')
        if n_par is None:
            n_par = max(1, min(self.lanes, len(sweeps)))
        res, failure = [], None
        try:
            for k, (az, el) in enumerate(sweeps):
                res.append(call(az, el, k % n_par))
        finally:
            for i in range(n_par):
                try:
                    self.wait(i)                      # (every lane is drained, whatever happened: no copy may outlive the call)
                except Exception as exc:              # noqa: BLE001  (re-raised below: the first failure of the scan)
                    failure = failure or exc
        if failure is not None:
            raise failure
        return res

    def _pass_over_sweeps(self, name, sweeps, call, per_sweep):
        """The sweeps of a scan reduced by call(az, el, phase, lane): per sweep (a list of results, the sweeps spread over the
        lanes), or all folded into ONE pass -- begun by the first sweep, finished by the last -- which stays on lane 0 as
        the statistics' passes stay on theirs: {name: the pass's result, 'sweeps': [what each call returned]}."""
        if per_sweep:
            return self._over_lanes(sweeps, lambda az, el, lane: call(az, el, 3, lane))
        phases = iter([(1 if k == 0 else 0) | (2 if k == len(sweeps) - 1 else 0) for k in range(len(sweeps))])
        res = self._over_lanes(sweeps, lambda az, el, lane: call(az, el, next(phases), lane), n_par=1)
        return {name: res[-1].pop(name), 'sweeps': res}

    def _sweep_groups(self, sweeps):
        """Consecutive sweeps whose launch sequence fits the memory budget (at least one sweep per group).  (`free` counts
        the work buffers the context holds already, cpol_mem_info: the same scan is grouped the same way on every call.)"""
        free, _, per_gate = self._ctx.mem_info()
        budget = self.sequence_memory_budget if self.sequence_memory_budget is not None else free // 3
        sub = self._cached('sub', lambda: quadrature.subbeams(self.__config))
        per_ray = per_gate * sub.n_sub * len(self.constants.RANGE_RADAR)
        groups, cur, used = [], [], 0
        for sw in sweeps:
            need = per_ray * len(np.asarray(sw[0]).reshape(-1))
            if cur and used + need > budget:
                groups.append(cur)
                cur, used = [], 0
            cur.append(sw)
            used += need
        if cur:
            groups.append(cur)
        return groups

    def _simulate_group(self, sweeps):
        """Sweeps as one launch sequence -> packaged per-sweep results (row slices of the group's arrays)."""
        az = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a, _ in sweeps])
        el = np.concatenate([np.asarray(e, dtype=np.float64).reshape(-1) for _, e in sweeps])
        res = self.simulate_rays(az, el)
        out, lo = [], 0
        for a, e in sweeps:
            hi = lo + len(np.asarray(a).reshape(-1))
            part = {k: (v[:, lo:hi] if k in ('model_vars',) else v[lo:hi]) if isinstance(v, np.ndarray) else v
                    for k, v in res.items()}
            out.append(self._package(part, a, e))
            lo = hi
        return out

    def _simulate_sweep(self, az, el, lane=0):
        """All rays of a sweep on this GPU."""
        return self.simulate_rays(az, el, lane=lane)

    def _dist_runner(self, group=None):
        """The operator's ShardedVolumeRunner (device buffers, the stream of the collectives) for the default
        process group, or one of its own for another `group` (kept until close())."""
        import torch
        from . import distributed as D
        if group is None:
            if self._runner is None:
                self._runner = D.ShardedVolumeRunner(torch.device('cuda', self.device), gather_to=self.gather_to,
                                                     slots=max(2, self.lanes + 1))
            return self._runner
        runners = self.__dict__.setdefault('_group_runners', {})
        if id(group) not in runners:
            import torch.distributed as dist
            members = dist.get_process_group_ranks(group)
            if dist.get_rank() not in members:
                raise ValueError('submit_volume(group=...): rank %d is not a member of the group (ranks %s)'
                                 % (dist.get_rank(), members))
            root = self.gather_to
            if root is not None:                  # (gather_to names a rank of the default group)
                if root not in members:
                    # (round-5 advisor: never re-root silently -- the scan would land on a rank nobody named)
                    raise ValueError('gather_to=%d is not a member of the group (ranks %s): results of a rooted '
                                     'gather must land on a rank of the group that computes them' % (root, members))
                root = dist.get_group_rank(group, root)
            runners[id(group)] = (group, D.ShardedVolumeRunner(torch.device('cuda', self.device), group=group,
                                                               gather_to=root, slots=max(2, self.lanes + 1)))
        return runners[id(group)][1]

    def _scan_fields(self, fields=None):
        """(name, dtype) of the arrays a distributed scan collects: all of them, or the subset named."""
        every = ([(k, np.float32) for k in RADAR_FIELDS] + [('dist', np.float32), ('heights', np.float32),
                 ('mask', np.float64), ('lats', np.float64), ('lons', np.float64)])
        if self.__config['doppler']['scheme'] in (1, 2, 3) and self.__config['radar'].get('type') != 'GPM':
            every.append(('RVEL', np.float64))               # (the spectrum itself is not gathered)
        if self.__config['integration'].get('terrain_visibility', 0) and self.__config['radar'].get('type') != 'GPM':
            every.append(('visibility', np.float64))
        if fields is None:
            return every
        known = dict(every)
        for k in fields:
            if k not in known:
                raise ValueError('distributed scans collect %s; %r is not one of them' % (sorted(known), k))
        return [(k, known[k]) for k in fields]

    def submit_volume(self, sweeps, fields=None, lane=0, group=None):
        """Queues a scan [(azimuths, elevations), ...] whose rays are sharded over the ranks of the default
        torch.distributed group (or of `group`) and returns at once: this rank's rays of ALL sweeps in one launch sequence
        on lane `lane`, ONE collective behind it (cosmo_pol_amd/distributed.py: all-gather, or a gather to
        rank `gather_to`), the device-to-host copy behind that.  -> PendingVolume: `wait()` gives the list of
        per-sweep result dicts (None on a rank that is not `gather_to`).  `fields`: the arrays to collect
        (default: all).  Scans submitted on different lanes overlap: the collective and the copy of one run
        beside the kernels of the next.  Every rank must submit the same scans in the same order."""
        if self.output_variables != 'only_radar':
            raise NotImplementedError('distributed sweeps return the radar observables only '
                                      "(use output_variables='only_radar')")
        n_gates = len(self.constants.RANGE_RADAR)
        ctx = self._lane(lane)

        def run_block(a, e, ptrs):
            self.simulate_rays(a, e, device_outputs=ptrs, lane=lane)
        return self._dist_runner(group).submit(run_block, ctx.stream_ptr(), sweeps, self._scan_fields(fields), n_gates,
                                               host_block=self._pool.take)

    def _simulate_volume_sharded(self, sweeps, lane=0):
        """All sweeps of a scan, the rays of every sweep sharded over the ranks (`submit_volume`, then
        wait).  -> list of per-sweep result dicts, or None on a rank other than `gather_to`."""
        res = self.submit_volume(sweeps, lane=lane).wait()
        self._lane(lane).synchronize()                          # deferred domain error, if any
        if res is None:
            return None
        sub = self._cached('sub', lambda: quadrature.subbeams(self.__config))
        for r in res:
            r['n_sub'] = sub.n_sub
        return res

    def _swath_sharded(self, az, el, coords, n_gates, range0, site, sub, traj, geo_t, dim, lane=0):
        """A spaceborne swath with its SCAN LINES sharded over the ranks in contiguous blocks:
        a rank runs the rays of its scan lines as one launch sequence into its block of the gather buffer,
        ONE collective, rows put into swath order on the device, one copy.  Every rank (or rank `gather_to`
        alone) gets the whole swath, bitwise equal to the single-GPU one.  (The swath geometry -- angles, first gates -- is
        computed by every rank: host work of milliseconds, cached per swath.)"""
        import torch.distributed as dist
        from . import distributed as D
        if self.output_variables != 'only_radar':
            raise NotImplementedError('distributed swaths return the radar observables only '
                                      "(use output_variables='only_radar')")
        n_scans, per_scan = dim
        fields = self._scan_fields()
        row = per_scan * n_gates                      # one row of the layout = one scan line
        lo, hi, _ = D.shard_bounds(n_scans, dist.get_world_size(), dist.get_rank())
        r0, r1 = lo * per_scan, hi * per_scan
        ctx = self._lane(lane)

        def run_block(_rows, _unused, ptrs):
            self._run_rays(az[r0:r1], el[r0:r1], coords[r0:r1], n_gates, range0, N.GEOM_SPACEBORNE,
                           device_outputs=ptrs, site=site[r0:r1], sub=sub, tables=(traj[r0:r1], geo_t[r0:r1]),
                           lane=lane)
        lines = [(np.arange(n_scans, dtype=np.float64), np.zeros(n_scans))]
        res = self._dist_runner().submit(run_block, ctx.stream_ptr(), lines, fields, row,
                                         host_block=self._pool.take).wait()
        ctx.synchronize()                                       # deferred domain error, if any
        if res is None:
            return None                                         # (gather_to: another rank holds the swath)
        out = {k: v.reshape(n_scans * per_scan, n_gates) for k, v in res[0].items()}
        out['n_sub'] = sub.n_sub
        return out

    def _package(self, res, az, el):
        fields = {}
        if self.output_variables in ('all', 'only_radar'):
            for k in RADAR_FIELDS + DOPPLER_FIELDS:
                if k in res:
                    fields[k] = res[k]
        if 'visibility' in res:                   # (integration/terrain_visibility: the visible share of the antenna pattern)
            fields['visibility'] = res['visibility']
        if self.output_variables in ('all', 'only_model'):
            for i, name in enumerate(self._staged_vars):
                fields[name] = res['model_vars'][i]
        return {'fields': fields, 'azimuth': np.asarray(az, dtype=float),
                'elevation': np.asarray(el, dtype=float), 'lats': res['lats'],
                'lons': res['lons'], 'mask': res['mask'], 'dist': res['dist'],
                'heights': res['heights']}

    def _finish_scan(self, scan):
        """RadarScan, or -- when `pyart_output` is set and Py-ART imports -- the reference's
        PyartRadop built from it (cosmo_pol/radar/pyart_wrapper.py:191-342)."""
        if getattr(self, 'pyart_output', False):
            from . import pyart_wrapper
            if pyart_wrapper.pyart_available():
                va = self.constants.VARRAY if self.__config['doppler']['scheme'] == 3 else None
                return pyart_wrapper.as_pyart_radar(scan, va)
            print('pyart_output requested but Py-ART does not import: returning a RadarScan')
        return scan

    def get_PPI(self, elevations, azimuths=None, az_step=None, az_start=0, az_stop=359):
        """Simulates PPI scan(s) (radar_operator.py:357-453); one sweep per
        elevation, returned as a RadarScan."""
        if not self._check_ready():
            return
        elevations, azimuths, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        sweeps = self._simulate_sweeps(sweeps)
        if sweeps is None:
            return None                       # distributed with gather_to: rank `gather_to` holds the scan
        return self._finish_scan(RadarScan('ppi', list(elevations), list(azimuths),
                                           self.constants.RANGE_RADAR, self.get_pos_and_time(), sweeps))

    def get_RHI(self, azimuths, elevations=None, elev_step=None, elev_start=0, elev_stop=90):
        """Simulates RHI scan(s) (radar_operator.py:455-549); one sweep per azimuth."""
        if not self._check_ready():
            return
        elevations, azimuths, sweeps = self._rhi_sweeps(azimuths, elevations, elev_step, elev_start, elev_stop)
        sweeps = self._simulate_sweeps(sweeps)
        if sweeps is None:
            return None
        return self._finish_scan(RadarScan('rhi', list(elevations), list(azimuths),
                                           self.constants.RANGE_RADAR, self.get_pos_and_time(), sweeps))

    # ------------------------------------------------------------------ superobservation scans
    def _superob_sweeps(self, sweeps, spec, keep_gates):
        """One pinned call per sweep over the lanes, one wait at the end: every sweep carries the bits of its own
        simulate_rays_superob(..., spec)."""
        return self._over_lanes(sweeps, lambda az, el, lane: self.simulate_rays_superob(az, el, spec, keep_gates=keep_gates,
                                                                                        pinned=True, lane=lane))

    def _ppi_sweeps(self, elevations, azimuths, az_step, az_start, az_stop):
        """get_PPI's defaults -> (elevations, azimuths, [(az, el) per sweep])"""
        if np.isscalar(elevations):
            elevations = [elevations]
        if az_step is None:
            az_step = self.__config['radar']['3dB_beamwidth']
        if azimuths is None or np.any(np.equal(azimuths, None)):
            if az_start > az_stop:
                azimuths = np.hstack((np.arange(az_start, 360., az_step),
                                      np.arange(0, az_stop + az_step, az_step)))
            else:
                azimuths = np.arange(az_start, az_stop + az_step, az_step)
        azimuths = np.asarray(azimuths, dtype=float)
        return elevations, azimuths, [(azimuths, np.full(len(azimuths), float(e))) for e in elevations]

    def _rhi_sweeps(self, azimuths, elevations, elev_step, elev_start, elev_stop):
        """get_RHI's defaults -> (elevations, azimuths, [(az, el) per sweep])"""
        if np.isscalar(azimuths):
            azimuths = [azimuths]
        if elevations is None or np.any(np.equal(elevations, None)):
            if elev_step is None:
                elev_step = self.__config['radar']['3dB_beamwidth']
            elevations = np.arange(elev_start, elev_stop + elev_step, elev_step)
        elevations = np.asarray(elevations, dtype=float)
        return elevations, azimuths, [(np.full(len(elevations), float(a)), elevations) for a in azimuths]

    def get_PPI_superob(self, elevations, spec, azimuths=None, az_step=None, az_start=0, az_stop=359, keep_gates=False):
        """The sweeps of get_PPI as superobservations: a list with one simulate_rays_superob(..., spec) result per elevation
        (res['superob']: window averages, counts, window coordinates).  Windows stay inside their sweep."""
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        return self._superob_sweeps(sweeps, spec, keep_gates)

    def get_RHI_superob(self, azimuths, spec, elevations=None, elev_step=None, elev_start=0, elev_stop=90, keep_gates=False):
        """The sweeps of get_RHI as superobservations: one result per azimuth (see get_PPI_superob)."""
        _, _, sweeps = self._rhi_sweeps(azimuths, elevations, elev_step, elev_start, elev_stop)
        return self._superob_sweeps(sweeps, spec, keep_gates)

    # ------------------------------------------------------------------ sweep histograms
    # (replaces in the reference: nothing -- its users pull every per-gate array to the host and call np.histogram2d there)
    def _doppler(self):
        """RVEL is simulated: a Doppler scheme, and no GPM-type radar."""
        conf = self.__config
        return conf['doppler']['scheme'] in (1, 2, 3) and conf['radar'].get('type') != 'GPM'

    def simulate_rays_histogram(self, azimuths, elevations, hist, keep_gates=False, phase=3, rays_per_block=0, device_outputs=None,
                                lane=0, pinned=False):
        """simulate_rays handing back a HISTOGRAM of its gates: `hist` is a histogram.Histogram, and a finishing call's result
        gains res['histogram'] = {'counts': {field: uint64 [n_blocks, (n_y + 2,) n_x + 2]}, 'edges': {field: the rounded
        edges}, 'ordinate_edges': ...} -- counted on the device behind the sweep's kernels (histogram.count states the rule,
        and the counts are exactly its counts of the call's own per-gate arrays).  Without `keep_gates` no per-gate radar field
        is produced for the host or copied; with it the result carries every array of simulate_rays, bit for bit.
        `phase`: bit 0 begins the lane's pass (clears), bit 1 finishes it (the counts come back); 0 only counts -- the sweeps
        of a volume, or a year of model states, fold into one CFAD.  `rays_per_block`: 0 one histogram of all rays, else a
        divisor of the rays: one histogram per block of rays.  `device_outputs`: its entry 'histogram' is {field: device pointer
        of the counts}.  (A method of its own: the keyword list of simulate_rays is pinned.)  ValueError for what the library
        refuses; NotImplementedError with a process group and for spaceborne geometry."""
        return self._simulate_rays(azimuths, elevations, device_outputs=device_outputs, lane=lane, pinned=pinned,
                                   product=HG.Counts(hist, keep_gates, phase, rays_per_block, self._doppler(), self.distributed))

    def simulate_rays_at_histogram(self, azimuths, elevations, times, hist, keep_gates=False, phase=3, rays_per_block=0,
                                   device_outputs=None, lane=0, pinned=False):
        """simulate_rays_at handing back a histogram: `hist`, `keep_gates`, `phase`, `rays_per_block` as for
        simulate_rays_histogram (ValueError when the rays fall into several groups of states)."""
        return self._simulate_rays_at(azimuths, elevations, times, device_outputs=device_outputs, lane=lane, pinned=pinned,
                                      product=HG.Counts(hist, keep_gates, phase, rays_per_block, self._doppler(), self.distributed))

    def simulate_rays_ensemble_histogram(self, azimuths, elevations, hist, members=None, per_member=True, keep_gates=False,
                                         phase=3, device_outputs=None, apply_sensitivity=True, lane=0, pinned=False):
        """simulate_rays_ensemble (form 'shared') handing back histograms: with `per_member` one histogram per member, in the
        order of `members` (the leading axis of the counts; rays_per_block = n_rays: each equals the member's own
        simulate_rays_histogram), without it one histogram of all members' gates.  The gate coordinates come once, and an
        ordinate 'heights' or 'dist' is every member's.  `keep_gates`: the per-member arrays of simulate_rays_ensemble come back
        too.  `phase`: as for simulate_rays_histogram; when `sequence_memory_budget` cuts the member list into several calls,
        per_member needs phase=3 (every chunk is a pass of its own and the blocks are joined), and the one histogram of all
        members folds the chunks into the pass.  NotImplementedError where simulate_rays_ensemble raises it."""
        return self._ensemble_reduced(azimuths, elevations, HG.Counts(hist, keep_gates, phase, 0, self._doppler(), self.distributed),
                                      'histograms', members, per_member, device_outputs, apply_sensitivity, lane, pinned)

    def _ensemble_reduced(self, azimuths, elevations, product, what, members, per_member, device_outputs, apply_sensitivity, lane,
                          pinned, radar=None, source=0):
        """An ensemble call (form 'shared') whose gates a histogram or a composite reduces: a block per member (`what` they
        are called), or one of all members' gates."""
        members = self._members_arg(members)
        coords = self._ensemble_coords()
        if radar is not None:
            coords = self._radar_arg(radar)
            if coords[2] > K.MAX_MODEL_HEIGHT:
                raise NotImplementedError('spaceborne geometry: use get_GPM_swath')
        if hasattr(product, 'set_plane'):
            self._set_plane(product, azimuths, elevations, coords, None, source, device_outputs, lane)
        sub = self._cached('sub', lambda: quadrature.subbeams(self.__config))
        rr = self.constants.RANGE_RADAR
        n_rays = len(np.asarray(azimuths).reshape(-1))
        chunks = self._shared_member_chunks(self._lane(lane), members, sub.n_sub * len(rr) * n_rays)
        name, phase = product.name, product.phase
        if len(chunks) > 1 and getattr(product, 'one_chunk', None):
            raise ValueError('simulate_rays_ensemble_%s: Probabilities needs the members in one chunk (%s)' % (name, product.one_chunk))
        if len(chunks) > 1 and device_outputs is not None:
            raise ValueError('simulate_rays_ensemble_%s: device outputs need the members in one chunk' % name)
        if len(chunks) > 1 and per_member and phase != 3:
            raise ValueError('simulate_rays_ensemble_%s: per-member %s of a member list cut into several calls need phase=3'
                             % (name, what))
        product.rays_per_block = n_rays if per_member else 0
        parts = []
        for i, chunk in enumerate(chunks):
            if not per_member and len(chunks) > 1:    # (one block of all members: the chunks fold into the pass)
                product.phase = (phase & 1 if i == 0 else 0) | (phase & 2 if i == len(chunks) - 1 else 0)
            parts.append(self._run_rays(azimuths, elevations, coords, len(rr), float(rr[0]), N.GEOM_GROUND_43,
                                        device_outputs=device_outputs, apply_sensitivity=apply_sensitivity, lane=lane,
                                        pinned=pinned and len(chunks) == 1, members=chunk, product=product))
        if len(parts) == 1 or device_outputs is not None:
            return parts[-1]
        once = _ONCE + ('n_sub',)
        out = {k: (parts[0][k] if k in once else np.concatenate([q[k] for q in parts])) for k in parts[0].keys() if k != name}
        if name in parts[-1]:
            out[name] = product.join([q.get(name) for q in parts], np.concatenate)
        return out

    def _histogram_sweeps(self, sweeps, hist, per_sweep, keep_gates, rays_per_block):
        """The sweeps of a scan counted: per sweep, or all folded into ONE pass (_pass_over_sweeps)."""
        return self._pass_over_sweeps('histogram', sweeps, lambda az, el, phase, lane: self.simulate_rays_histogram(
            az, el, hist, keep_gates=keep_gates, phase=phase, rays_per_block=rays_per_block, pinned=True, lane=lane), per_sweep)

    def get_PPI_histogram(self, elevations, hist, azimuths=None, az_step=None, az_start=0, az_stop=359, per_sweep=False,
                          keep_gates=False):
        """The sweeps of get_PPI counted into a histogram.  By default ALL sweeps fold into one pass (the volume's CFAD):
        {'histogram': as for simulate_rays_histogram, 'sweeps': [what each call returned: the per-gate arrays with
        keep_gates]}.  With `per_sweep` a list with one simulate_rays_histogram(..., hist) result per elevation, the sweeps
        spread over the lanes."""
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        return self._histogram_sweeps(sweeps, hist, per_sweep, keep_gates, 0)

    def get_RHI_histogram(self, azimuths, hist, elevations=None, elev_step=None, elev_start=0, elev_stop=90, per_sweep=False,
                          keep_gates=False):
        """The sweeps of get_RHI counted into a histogram: one pass over all azimuths, or one result per azimuth (see
        get_PPI_histogram)."""
        _, _, sweeps = self._rhi_sweeps(azimuths, elevations, elev_step, elev_start, elev_stop)
        return self._histogram_sweeps(sweeps, hist, per_sweep, keep_gates, 0)

    # ------------------------------------------------------------------ gridded composites
    # (replaces in the reference: nothing -- its users pull every per-gate array to the host, compute per gate where it lies and
    # scatter with np.maximum.at)
    def simulate_rays_composite(self, azimuths, elevations, spec, keep_gates=False, phase=3, rays_per_block=0, device_outputs=None,
                                lane=0, pinned=False, radar=None, source=0):
        """simulate_rays handing back MAPS of its gates on a radar-centred grid: `spec` is a composite.Composite, and a finishing
        call's result gains res['composite'] = {'values': {field: {plane: float32 [n_blocks, n_y, n_x]}}, 'count': {field: uint64
        [n_blocks, n_y, n_x]}, 'x_edges', 'y_edges'} -- the column maximum, the lowest gate and the echo tops, reduced on the
        device behind the sweep's kernels (composite.compose / composite.finish state the rule, and the maps are exactly theirs of
        the call's own per-gate arrays, `dist`, `heights` and azimuths).  Without `keep_gates` no per-gate radar field is
        produced for the host or copied; with it the result carries every array of simulate_rays, bit for bit.
        `phase`: bit 0 begins the lane's pass, bit 1 finishes it (the maps come back); 0 only folds -- the sweeps of a volume
        fold into one composite.  `rays_per_block`: 0 one map of all rays, else a divisor of the rays: one map per block of rays.
        `device_outputs`: its entry 'composite' is {'values': {field: device pointer}, 'count': device pointer} (on a gate plane
        also 'gate_x', 'gate_y': device pointers of float64 [n_rays, n_gates]).
        `radar`: (lat, lon, alt) in place of config['radar']['coords'] for this call alone -- band, beamwidth, range and
        resolution stay the configuration's, so the radars of a network under one operator differ in position only; `source`
        (0 ... 254): this call's number in the source_of_* planes of a spec with 'source'.  On a plane other than 'radar'
        (composite.Composite(plane=)) the call hands the library per-gate coordinates made on the host from the gate
        coordinates of its table set (composite.plane_xy), cached with them; the first time a geometry is seen this costs one
        plain call on the lane (every time without reuse_device_tables or with host ray paths).
        ValueError for what the library refuses; NotImplementedError with a process group and for spaceborne geometry."""
        return self._simulate_rays(azimuths, elevations, device_outputs=device_outputs, lane=lane, pinned=pinned,
                                   product=CP.Maps(spec, keep_gates, phase, rays_per_block, self.distributed), radar=radar, source=source)

    def simulate_rays_at_composite(self, azimuths, elevations, times, spec, keep_gates=False, phase=3, rays_per_block=0,
                                   device_outputs=None, lane=0, pinned=False, radar=None, source=0):
        """simulate_rays_at handing back a composite: `spec`, `keep_gates`, `phase`, `rays_per_block`, `radar` (the radars of a
        network differ in position only) and `source` as for simulate_rays_composite (ValueError when the rays fall into
        several groups of states)."""
        return self._simulate_rays_at(azimuths, elevations, times, device_outputs=device_outputs, lane=lane, pinned=pinned,
                                      product=CP.Maps(spec, keep_gates, phase, rays_per_block, self.distributed), radar=radar,
                                      source=source)

    def simulate_rays_ensemble_composite(self, azimuths, elevations, spec, members=None, per_member=True, keep_gates=False,
                                         phase=3, device_outputs=None, apply_sensitivity=True, lane=0, pinned=False, radar=None,
                                         source=0):
        """simulate_rays_ensemble (form 'shared') handing back composites: with `per_member` one map per member, in the order
        of `members` (the leading axis of every plane; rays_per_block = n_rays: each equals the member's own
        simulate_rays_composite), without it one map of all members' gates.  The gate coordinates come once.  `keep_gates`:
        the per-member arrays of simulate_rays_ensemble come back too.  `phase`: as for simulate_rays_composite; when
        `sequence_memory_budget` cuts the member list into several calls, per_member needs phase=3 (every chunk is a pass of its
        own and the blocks are joined), and the one map of all members folds the chunks into the pass.  `radar` (the radars of a
        network differ in position only) and `source`: as for simulate_rays_composite.  NotImplementedError where
        simulate_rays_ensemble raises it."""
        return self._ensemble_reduced(azimuths, elevations, CP.Maps(spec, keep_gates, phase, 0, self.distributed), 'maps', members,
                                      per_member, device_outputs, apply_sensitivity, lane, pinned, radar=radar, source=source)

    def get_PPI_composite(self, elevations, spec, azimuths=None, az_step=None, az_start=0, az_stop=359, per_sweep=False,
                          keep_gates=False):
        """The sweeps of get_PPI composed onto a map.  By default ALL sweeps fold into one pass (the volume's composite):
        {'composite': as for simulate_rays_composite, 'sweeps': [what each call returned: the per-gate arrays with keep_gates]}.
        With `per_sweep` a list with one simulate_rays_composite(..., spec) result per elevation, the sweeps spread over the
        lanes.  (An RHI has no such entry: its plan view is a line.)"""
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        return self._pass_over_sweeps('composite', sweeps, lambda az, el, phase, lane: self.simulate_rays_composite(
            az, el, spec, keep_gates=keep_gates, phase=phase, pinned=True, lane=lane), per_sweep)

    # ------------------------------------------------------------------ neighbourhood verification of composites
    # (replaces in the reference: nothing -- its users grid the radials, threshold both maps and run box filters on the host)
    def _fss_product(self, spec, observed, domain, device_outputs, keep_gates, phase, rays_per_block):
        """The product object of a composite call with scores; `observed` and `domain` checked (host arrays), or device pointers
        under device_outputs['composite'] and `observed` None.  `spec`: a neighbourhood.Fractions, or an objects.Objects over
        one: the scores with the object cells of the same binary maps (objects.Cells), or a neighbourhood.Probabilities over
        one: the scores with the neighbourhood ensemble probabilities of the blocks (neighbourhood.EnsembleScores)."""
        cells, spec = (spec, spec.fractions) if isinstance(spec, OB.Objects) else (None, spec)
        prob, spec = (spec, spec.fractions) if isinstance(spec, NB.Probabilities) else (None, spec)
        if not isinstance(spec, NB.Fractions):
            raise ValueError('spec: a cosmo_pol_amd.neighbourhood.Fractions, got %r' % (spec,))
        entry = (device_outputs or {}).get('composite', {})
        if int(phase) & 2:
            if (observed is None) == (entry.get('observed') is None):
                raise ValueError("a Fractions call needs the observed map (a NumPy array), or with device_outputs the device "
                                 "pointer device_outputs['composite']['observed'], and not both")
            if observed is not None and device_outputs is not None:
                raise ValueError("with device_outputs the observed map is a device pointer under device_outputs['composite']['observed']")
            if observed is None and domain is not None:
                raise ValueError("with device_outputs the domain is a device pointer under device_outputs['composite']['domain']")
        if observed is not None:
            observed, domain = NB.check_maps(spec, observed, domain)
        if cells is not None:
            return OB.Cells(cells, observed, domain, keep_gates, phase, rays_per_block, self.distributed)
        if prob is not None:
            return NB.EnsembleScores(prob, observed, domain, keep_gates, phase, rays_per_block, self.distributed)
        return NB.Scores(spec, observed, domain, keep_gates, phase, rays_per_block, self.distributed)

    def simulate_rays_composite_fss(self, azimuths, elevations, spec, observed, domain=None, keep_gates=False, phase=3,
                                    rays_per_block=0, device_outputs=None, lane=0, pinned=False, radar=None, source=0):
        """simulate_rays_composite with the finished plane SCORED against an observed map on the device: `spec` is a
        neighbourhood.Fractions (its composite, the field and plane to score, thresholds and radii), `observed` float32
        [n_y, n_x] on the composite's grid in the field's linear units (NaN = no echo or no data), `domain` an optional uint8
        [n_y, n_x] mask of the verification domain.  A finishing call's res['composite'] gains 'fractions': {'diff2' |
        'forecast2' | 'observed2': uint64 [n_blocks, n_thr, n_radii], 'n_forecast' | 'n_observed' | 'n_domain': uint64
        [n_blocks, n_thr], 'thresholds', 'radii'} -- exactly neighbourhood.sums of the map the same call returns;
        neighbourhood.fss, bias and contingency make the scores of them.  A pass is scored only by the call that finishes it.
        With an objects.Objects (over a Fractions) as `spec` it gains 'objects' too: the object cells of the same binary maps,
        of every block and once of the observed map, exactly objects.cells of the map the same call returns ({'n_objects',
        'first', 'area', 'sum_x', 'sum_y', 'bbox', 'peak', 'peak_cell', 'labels' when asked, 'observed': the same,
        'connectivity', 'min_area', 'thresholds'}); device_outputs['composite'] may then carry 'n_objects', 'table' and 'labels'.
        With Objects(match=True) 'objects' also holds the overlap pieces of every block's objects with the observed ones
        ('pieces', 'covered', 'covered_observed': objects.py, MATCH), and the entry may carry 'n_pieces', 'pieces' and 'covered'.
        With Objects(track=True, ...) and at least two blocks 'objects' also holds 'track': every block's objects followed into
        the next block ('correlation', 'shift', 'n_pieces', 'pieces', 'covered': objects.py, TRACK; objects.links, tracks and
        motion read it), and the entry may carry 'track_correlation', 'track_shift', 'track_n_pieces', 'track_pieces' and
        'track_covered'; a call that yields one block is a ValueError.
        With a neighbourhood.Probabilities (over a Fractions; over an Objects it is a ValueError: not built) as `spec` it gains
        'probabilities': the neighbourhood ensemble probabilities of the call's blocks, exactly neighbourhood.ensemble_sums of
        the maps the same call returns ({'diff2' | 'forecast2' | 'observed2': uint64 [n_thr, n_radii], 'reliability': uint64
        [n_thr, n_radii, n_blocks + 1, 2], 'member_sum' | 'member_any': uint32 [n_thr, n_radii, n_y, n_x] when asked,
        'n_blocks', 'thresholds', 'radii'}); neighbourhood.fss, nep, nmep, brier, reliability_curve and roc read it, and the
        entry may carry 'prob_sums', 'reliability', 'member_sum' and 'member_any'.
        The other keywords are those of simulate_rays_composite.  `device_outputs`: its entry 'composite' may carry 'observed',
        'domain', 'sums' and 'totals' as device pointers (`observed` stays None).  ValueError for an observed map or a domain of
        a wrong shape or dtype and for what the library refuses.  `radar` (the radars of a network under one operator differ in
        position only) and `source`: as for simulate_rays_composite."""
        return self._simulate_rays(azimuths, elevations, device_outputs=device_outputs, lane=lane, pinned=pinned,
                                   product=self._fss_product(spec, observed, domain, device_outputs, keep_gates, phase, rays_per_block),
                                   radar=radar, source=source)

    def simulate_rays_at_composite_fss(self, azimuths, elevations, times, spec, observed, domain=None, keep_gates=False, phase=3,
                                       rays_per_block=0, device_outputs=None, lane=0, pinned=False, radar=None, source=0):
        """simulate_rays_at_composite with scores: `spec`, `observed`, `domain` as for simulate_rays_composite_fss; `radar` (the
        radars of a network differ in position only) and `source` as for simulate_rays_composite."""
        return self._simulate_rays_at(azimuths, elevations, times, device_outputs=device_outputs, lane=lane, pinned=pinned,
                                      product=self._fss_product(spec, observed, domain, device_outputs, keep_gates, phase, rays_per_block),
                                      radar=radar, source=source)

    def simulate_rays_ensemble_composite_fss(self, azimuths, elevations, spec, observed, domain=None, members=None, per_member=True,
                                             keep_gates=False, phase=3, device_outputs=None, apply_sensitivity=True, lane=0,
                                             pinned=False, radar=None, source=0):
        """simulate_rays_ensemble_composite with scores: with `per_member` one row of scores per member (the leading axis of
        every array of 'fractions', in the order of `members`; each equals the member's own simulate_rays_composite_fss),
        without it the scores of the one map of all members' gates.  `spec`, `observed`, `domain` as for
        simulate_rays_composite_fss: with a neighbourhood.Probabilities the members are the blocks of res['composite']
        ['probabilities'] (NEP, NMEP, the ensemble FSS, the reliability table), with per_member=False there is one block, and a
        member list that `sequence_memory_budget` cuts into several calls is a ValueError; the rest (`radar`, `source`: the radars of a network differ in position only) as for
        simulate_rays_ensemble_composite.  An Objects with track=True is a ValueError: the blocks here are members, not times."""
        if isinstance(spec, OB.Objects) and spec.track:
            raise ValueError('track: the blocks of an ensemble call are members, not times')
        return self._ensemble_reduced(azimuths, elevations, self._fss_product(spec, observed, domain, device_outputs, keep_gates, phase, 0),
                                      'maps', members, per_member, device_outputs, apply_sensitivity, lane, pinned, radar=radar,
                                      source=source)

    def get_PPI_composite_fss(self, elevations, spec, observed, domain=None, azimuths=None, az_step=None, az_start=0, az_stop=359,
                              per_sweep=False, keep_gates=False):
        """get_PPI_composite with scores.  By default the volume folds into one pass, which is scored ONCE, at its end:
        {'composite': as for simulate_rays_composite_fss, 'sweeps': [...]}.  With `per_sweep` a list with one
        simulate_rays_composite_fss(..., spec, observed) result per elevation."""
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        return self._pass_over_sweeps('composite', sweeps, lambda az, el, phase, lane: self.simulate_rays_composite_fss(
            az, el, spec, observed, domain=domain, keep_gates=keep_gates, phase=phase, pinned=True, lane=lane), per_sweep)

    # ------------------------------------------------------------------ network composites
    # (replaces in the reference: nothing -- it simulates one radar per run)
    def _network_sweeps(self, radars, cspec, elevations, azimuths, az_step, az_start, az_stop):
        """[(az, el, radar, source)] of every elevation of every radar, and the checks of a network call."""
        radars = [self._radar_arg(r) for r in radars]
        if not radars:
            raise ValueError('radars: at least one (lat, lon, alt)')
        if len(radars) > CP.NO_SOURCE:
            raise ValueError('radars: at most %d (the source of a cell is one byte), got %d' % (CP.NO_SOURCE, len(radars)))
        if not isinstance(cspec, CP.Composite):
            raise ValueError('spec: a cosmo_pol_amd.composite.Composite, got %r' % (cspec,))
        if len(radars) > 1 and not cspec.gate_plane:
            raise ValueError("the plane 'radar' is centred on ONE radar: a network needs plane='geographic', 'model' or a callable")
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        with_source = CP.SOURCE in cspec.products
        return [(az, el, r, i if with_source else 0) for i, r in enumerate(radars) for az, el in sweeps], len(sweeps)

    def _network_pass(self, sweeps, per_radar, call):
        """Every sweep of every radar folded into ONE pass on lane 0 (_pass_over_sweeps), scored -- if at all -- once, at its end."""
        which = iter(sweeps)

        def one(az, el, phase, lane):
            _, _, radar, source = next(which)
            return call(az, el, phase, lane, radar, source)
        out = self._pass_over_sweeps('composite', [(az, el) for az, el, _, _ in sweeps], one, False)
        flat = out['sweeps']
        out['sweeps'] = [flat[i:i + per_radar] for i in range(0, len(flat), per_radar)]
        return out

    def get_network_composite(self, radars, elevations, spec, azimuths=None, az_step=None, az_start=0, az_stop=359, keep_gates=False):
        """The PPI volumes of SEVERAL radars composed onto one map: `radars` is a list of (lat, lon, alt), each scanned at
        `elevations` (the azimuths as for get_PPI) with the configuration's band, beamwidth, range and resolution -- the radars
        of a network under one operator differ in position only.  `spec`: a composite.Composite on the plane 'geographic',
        'model' or a callable (ValueError for 'radar' with more than one radar, and for more than 255 radars).  Every elevation
        of every radar folds into one pass on lane 0; with the product 'source' the planes source_of_max / source_of_lowest
        hold the index in `radars` of the radar that supplied the cell.  Returns {'composite': as for simulate_rays_composite,
        'sweeps': [per radar [per elevation: what the call returned, the per-gate arrays with keep_gates]]}."""
        sweeps, per_radar = self._network_sweeps(radars, spec, elevations, azimuths, az_step, az_start, az_stop)
        return self._network_pass(sweeps, per_radar, lambda az, el, phase, lane, radar, source: self.simulate_rays_composite(
            az, el, spec, keep_gates=keep_gates, phase=phase, pinned=True, lane=lane, radar=radar, source=source))

    def get_network_composite_fss(self, radars, elevations, spec, observed, domain=None, azimuths=None, az_step=None, az_start=0,
                                  az_stop=359, keep_gates=False):
        """get_network_composite with scores: `spec` is a neighbourhood.Fractions over the network's composite, `observed` and
        `domain` as for simulate_rays_composite_fss.  The pass is scored ONCE, at its end, against the observed network
        composite: res['composite']['fractions'] (and 'objects' with an objects.Objects)."""
        if not isinstance(spec, (NB.Fractions, OB.Objects, NB.Probabilities)):
            raise ValueError('spec: a cosmo_pol_amd.neighbourhood.Fractions, got %r' % (spec,))
        sweeps, per_radar = self._network_sweeps(radars, spec.composite, elevations, azimuths, az_step, az_start, az_stop)
        return self._network_pass(sweeps, per_radar, lambda az, el, phase, lane, radar, source: self.simulate_rays_composite_fss(
            az, el, spec, observed, domain=domain, keep_gates=keep_gates, phase=phase, pinned=True, lane=lane, radar=radar,
            source=source))

    # ------------------------------------------------------------------ spectrum moments scans
    def _moments_sweeps(self, sweeps, moments, keep_spectrum):
        """One pinned call per sweep over the lanes, one wait at the end: every sweep carries the bits of its own
        simulate_rays_moments(..., moments)."""
        return self._over_lanes(sweeps, lambda az, el, lane: self.simulate_rays_moments(az, el, moments, keep_spectrum=keep_spectrum,
                                                                                        pinned=True, lane=lane))

    def get_PPI_moments(self, elevations, moments, azimuths=None, az_step=None, az_start=0, az_stop=359, keep_spectrum=False):
        """The sweeps of get_PPI with spectrum moments: a list with one simulate_rays_moments(..., moments) result per
        elevation (res['moments']), the sweeps spread over the lanes."""
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        return self._moments_sweeps(sweeps, moments, keep_spectrum)

    def get_RHI_moments(self, azimuths, moments, elevations=None, elev_step=None, elev_start=0, elev_stop=90, keep_spectrum=False):
        """The sweeps of get_RHI with spectrum moments: one result per azimuth (see get_PPI_moments)."""
        _, _, sweeps = self._rhi_sweeps(azimuths, elevations, elev_step, elev_start, elev_stop)
        return self._moments_sweeps(sweeps, moments, keep_spectrum)

    # ------------------------------------------------------------------ hydrometeor contributions
    # (replaces in the reference: nothing -- it folds the per-species sums and hands back the totals; its users re-run the sweep
    # once per species with the others zeroed)
    def _species_product(self, spec, keep_gates):
        if not self._check_ready():
            raise ValueError('no model loaded')
        return SP.Contributions(spec, self._staged_hydro, keep_gates, self.distributed)

    def simulate_rays_species(self, azimuths, elevations, spec, keep_gates=True, device_outputs=None, lane=0, pinned=False):
        """simulate_rays handing back HYDROMETEOR CONTRIBUTIONS: `spec` is a species.Species, and the result gains
        res['species'] = {'names': the species in slot order, one float32 [n_hydro, n_rays, n_gates] array per requested field
        (what the species alone gives: linear units, NaN where it has no item or the gate is censored; ZDR is the intrinsic
        ratio, not attenuated), 'dominant' (uint8, the slot with the largest ZH, 255: none), 'present' (uint8, bit j: slot j
        contributes), 'share' (float32, the dominant species' part of the sum of the species' ZH), and with `raw` 'sz'
        [n_rays, n_gates, n_hydro, 12]: the per-species sums themselves} -- made on the device behind the sweep's kernels
        (species.fields_of states the rule, and the arrays are exactly its result on the call's own 'sz' and ZH).  The per-gate
        arrays of the call have the bits of simulate_rays; the call takes the general launch sequence (a single-beam sweep gives
        up its fast kernels: they do not form the per-species rows).  Without `keep_gates` no per-gate radar field is produced for
        the host or copied.  `device_outputs`: its entry 'species' is {array name: device pointer}.  (A method of its own: the
        keyword list of simulate_rays is pinned.)  ValueError for what the library refuses; NotImplementedError with a process
        group, for spaceborne geometry and for ensemble calls."""
        return self._simulate_rays(azimuths, elevations, device_outputs=device_outputs, lane=lane, pinned=pinned,
                                   product=self._species_product(spec, keep_gates))

    def simulate_rays_at_species(self, azimuths, elevations, times, spec, keep_gates=True, device_outputs=None, lane=0, pinned=False):
        """simulate_rays_at handing back hydrometeor contributions: `spec` and `keep_gates` as for simulate_rays_species
        (ValueError when the rays fall into several groups of states)."""
        return self._simulate_rays_at(azimuths, elevations, times, device_outputs=device_outputs, lane=lane, pinned=pinned,
                                      product=self._species_product(spec, keep_gates))

    def _species_sweeps(self, sweeps, spec, keep_gates):
        """One pinned call per sweep over the lanes, one wait at the end: every sweep carries the bits of its own
        simulate_rays_species(..., spec)."""
        return self._over_lanes(sweeps, lambda az, el, lane: self.simulate_rays_species(az, el, spec, keep_gates=keep_gates,
                                                                                        pinned=True, lane=lane))

    def get_PPI_species(self, elevations, spec, azimuths=None, az_step=None, az_start=0, az_stop=359, keep_gates=True):
        """The sweeps of get_PPI with hydrometeor contributions: a list with one simulate_rays_species(..., spec) result per
        elevation (res['species']), the sweeps spread over the lanes."""
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        return self._species_sweeps(sweeps, spec, keep_gates)

    def get_RHI_species(self, azimuths, spec, elevations=None, elev_step=None, elev_start=0, elev_stop=90, keep_gates=True):
        """The sweeps of get_RHI with hydrometeor contributions: one result per azimuth (see get_PPI_species)."""
        _, _, sweeps = self._rhi_sweeps(azimuths, elevations, elev_step, elev_start, elev_stop)
        return self._species_sweeps(sweeps, spec, keep_gates)

    # ------------------------------------------------------------------ ensemble statistics scans
    def _ensemble_stats_sweeps(self, sweeps, stats, members, observations=None):
        """One pinned simulate_rays_ensemble_stats per sweep over the lanes, one wait at the end: every sweep's pass stays on
        its lane and carries the bits of its own call.  `observations`: one dict per sweep (an EnsembleVerification)."""
        members = self._members_arg(members)
        if observations is None:
            return self._over_lanes(sweeps, lambda az, el, lane: self.simulate_rays_ensemble_stats(az, el, stats, members=members,
                                                                                                   pinned=True, lane=lane))
        observations = list(observations)
        if len(observations) != len(sweeps):
            raise ValueError('observations: one dict per sweep (%d sweeps, got %d)' % (len(sweeps), len(observations)))
        obs = iter(observations)
        return self._over_lanes(sweeps, lambda az, el, lane: self.simulate_rays_ensemble_verify(az, el, stats, next(obs), members=members,
                                                                                                pinned=True, lane=lane))

    def get_PPI_ensemble_stats(self, elevations, stats, azimuths=None, az_step=None, az_start=0, az_stop=359, members=None):
        """The sweeps of get_PPI reduced over the ensemble: a list with one simulate_rays_ensemble_stats(..., stats) result
        per elevation (res['stats']), the sweeps spread over the lanes."""
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        return self._ensemble_stats_sweeps(sweeps, stats, members)

    def get_PPI_ensemble_verify(self, elevations, stats, observations, azimuths=None, az_step=None, az_start=0, az_stop=359,
                                members=None):
        """get_PPI_ensemble_stats with an ensemble_verify.EnsembleVerification: `observations` is a list with one {field:
        [n_rays, n_gates]} per elevation, and every result is that of simulate_rays_ensemble_verify."""
        if not isinstance(stats, EV.EnsembleVerification):
            raise ValueError('stats: a cosmo_pol_amd.ensemble_verify.EnsembleVerification, got %r' % (stats,))
        _, _, sweeps = self._ppi_sweeps(elevations, azimuths, az_step, az_start, az_stop)
        return self._ensemble_stats_sweeps(sweeps, stats, members, observations)

    def get_RHI_ensemble_stats(self, azimuths, stats, elevations=None, elev_step=None, elev_start=0, elev_stop=90, members=None):
        """The sweeps of get_RHI reduced over the ensemble: one result per azimuth (see get_PPI_ensemble_stats)."""
        _, _, sweeps = self._rhi_sweeps(azimuths, elevations, elev_step, elev_start, elev_stop)
        return self._ensemble_stats_sweeps(sweeps, stats, members)

    def get_RHI_ensemble_verify(self, azimuths, stats, observations, elevations=None, elev_step=None, elev_start=0, elev_stop=90,
                                members=None):
        """get_RHI_ensemble_stats with an ensemble_verify.EnsembleVerification: one dict of observations per azimuth (see
        get_PPI_ensemble_verify)."""
        if not isinstance(stats, EV.EnsembleVerification):
            raise ValueError('stats: a cosmo_pol_amd.ensemble_verify.EnsembleVerification, got %r' % (stats,))
        _, _, sweeps = self._rhi_sweeps(azimuths, elevations, elev_step, elev_start, elev_stop)
        return self._ensemble_stats_sweeps(sweeps, stats, members, observations)

    def get_VPROF(self):
        """90-degree vertical profile (the reference's version is broken as
        shipped, radar_operator.py:311-354; implemented as a one-ray RHI)."""
        if not self._check_ready():
            return
        return self.get_RHI(azimuths=[0.], elevations=[90.])

    def get_GPM_swath(self, GPM_file, band='Ku'):
        """Simulates a GPM-DPR swath (radar_operator.py:551-677, intended behaviour;
        the reference's version is dead as shipped).  `GPM_file`: path
        of a DPR HDF5 file (needs h5py) or a dict with Latitude, Longitude [N, M],
        scLat, scLon, dprAlt [N], scPos [N, 3].  Returns a SimulatedGPM."""
        from . import gpm
        if not self._check_ready():
            return
        if self.__config['integration'].get('terrain_shadow', 0):
            raise NotImplementedError('get_GPM_swath: integration/terrain_shadow is not for swaths (their gates run from the '
                                      'satellite downward)')
        swath = gpm.read_swath(GPM_file, band)
        freq, res_m = gpm.band_settings(band)
        saved = self.config
        conf = self.config
        conf['radar']['frequency'] = freq
        conf['radar']['3dB_beamwidth'] = K.GPM_3DB_BEAMWIDTH
        conf['radar']['sensitivity'] = float(K.GPM_SENSITIVITY)
        conf['radar']['type'] = 'GPM'
        conf['radar']['radial_resolution'] = res_m
        try:
            self.config = conf                   # reloads the tables of the new frequency
            # everything below depends on the swath geometry and the band only: kept for the last few
            # swaths (a Ku and a Ka call on the same file, repeated calls on one overpass)
            import hashlib
            hk = hashlib.blake2b(digest_size=16)
            for name in ('Latitude', 'Longitude', 'scLat', 'scLon', 'dprAlt', 'scPos'):
                hk.update(np.ascontiguousarray(swath[name], dtype=np.float64).tobytes())
            hk.update(repr(sorted(self.__config['integration'].items(), key=str)).encode())
            gkey = (hk.hexdigest(), band, self._staged_serial)
            gcache = self.__dict__.setdefault('_gpm_cache', {})  # (survives the configuration switches of this call)
            cached = gcache.get(gkey)
            if cached is None:
                az, el, rng, sat = gpm.swath_angles(swath)
                dim = az.shape
                az, el, rng = az.ravel(), el.ravel(), rng.ravel()
                coords = np.repeat(sat, dim[1], axis=0)                      # one site per ray
                sub = quadrature.subbeams(self.__config)
                traj, geo_t = geo.ray_tables(coords, az, el, sub)
                n_rays = len(az)
                # candidate gates: np.arange(res/2, slant range, res) (atm_refraction.py:252)
                n_cand = np.maximum(np.ceil((rng - res_m / 2.) / res_m), 0).astype(np.int32)
                sin_u1, cos_u1, _ = geo.radar_site_constants(coords)
                site = np.zeros((n_rays, 8))
                site[:, 0], site[:, 1], site[:, 2], site[:, 3] = sin_u1, cos_u1, coords[:, 1], coords[:, 2]
                site[:, 4] = geo.get_earth_radius(coords[:, 0])              # quirk Q1 (degrees as radians)
                p = N.SweepParams()
                p.n_rays, p.n_vnodes = n_rays, len(sub.pts_ver)
                p.range0, p.range_step = res_m / 2., float(res_m)
                first = self._ctx.spaceborne_first_gate(p, traj, site, n_cand, K.MAX_MODEL_HEIGHT)
                k0 = first[:, sub.sub_v[sub.central]]
                n_kept = (n_cand - k0).astype(np.int64)
                site[:, 5], site[:, 6] = k0, n_kept
                n_gates = int(max(1, n_kept.max()))
                cached = (az, el, rng, dim, coords, sub, traj, geo_t, site, n_kept, n_gates)
                with self._lock:
                    for k in list(gcache)[:-3]:
                        del gcache[k]
                    gcache[gkey] = cached
            az, el, rng, dim, coords, sub, traj, geo_t, site, n_kept, n_gates = cached
            if self.distributed:
                res = self._swath_sharded(az, el, coords, n_gates, res_m / 2., site, sub, traj, geo_t, dim)
                if res is None:
                    return None               # gather_to: another rank holds the swath
            else:
                res = self._run_rays(az, el, coords, n_gates, res_m / 2., N.GEOM_SPACEBORNE,
                                     site=site, sub=sub, tables=(traj, geo_t))
            fields = {}
            if self.output_variables in ('all', 'only_radar'):
                for k in RADAR_FIELDS:
                    fields[k] = res[k]
            if self.output_variables in ('all', 'only_model'):
                for i, name in enumerate(self._staged_vars):
                    fields[name] = res['model_vars'][i]
            out = gpm.SimulatedGPM(fields, res['mask'], res['lats'], res['lons'], n_kept, dim, band)
            out.raw = res
            out.n_kept = n_kept.reshape(dim)
            out.azimuths, out.elevations, out.ranges = (az.reshape(dim), el.reshape(dim),
                                                        rng.reshape(dim))
            return out
        finally:
            self.config = saved
