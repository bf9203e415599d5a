"""ctypes binding of libcosmo_pol_hip.so (C ABI: include/cosmo_pol_amd.h).

There is NO CPU fallback: if the HIP library is missing or fails to load the
import raises, and every entry point raises on a non-zero status.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libcosmo_pol_hip.so')

CPOL_MAX_VARS = 24
CPOL_MAX_HYDRO = 8
CPOL_MAX_PAR = 6
N_SZ = 12
MAX_GATES = 5460                                    # CPOL_MAX_GATES: gates of a ray (the three scan rows in 64 KB of LDS)

PSD_GAMMA, PSD_ICE_FIELD, PSD_MELTING = 0, 1, 2
(RULE_RAIN_1MOM, RULE_SNOW_1MOM, RULE_GRAUPEL_1MOM, RULE_TWO_MOMENT, RULE_ICE_1MOM,
 RULE_MELTING_SNOW, RULE_MELTING_GRAUPEL) = range(7)
Q_MODEL, Q_MELT_SNOW, Q_MELT_GRAUPEL = 0, 1, 2
GEOM_GROUND_43, GEOM_SPACEBORNE, GEOM_HOST_PATHS = 0, 1, 2
DEBUG_EXACT_SUBBEAMS = 1

ERR_HIP, ERR_ARG, ERR_DOMAIN, ERR_NOMEM = -1, -2, -3, -4


class HydroDesc(C.Structure):
    _fields_ = [
        ('psd_family', C.c_int32), ('rule', C.c_int32), ('q_source', C.c_int32),
        ('var_q', C.c_int32), ('var_qn', C.c_int32), ('var_t', C.c_int32),
        ('n_e', C.c_int32), ('n_t', C.c_int32), ('n_d', C.c_int32),
        ('second_axis_f64', C.c_int32),
        ('e_lo', C.c_float), ('e_step', C.c_float), ('t_lo', C.c_float), ('t_step', C.c_float),
        ('dD', C.c_double),
        ('a', C.c_double), ('b', C.c_double), ('alpha', C.c_double), ('beta', C.c_double),
        ('mu', C.c_double), ('nu', C.c_double),
        ('lambda_factor', C.c_double), ('ntot_factor', C.c_double), ('vel_factor', C.c_double),
        ('n0_fixed', C.c_double), ('x_min', C.c_double), ('x_max', C.c_double),
        ('c_n0', C.c_double), ('c_lam', C.c_double),
        ('lam_exponent', C.c_double), ('n0_exponent', C.c_double),
        ('r_a', C.c_double), ('r_b', C.c_double), ('r_alpha', C.c_double), ('r_beta', C.c_double),
        ('r_n0', C.c_double), ('r_mu', C.c_double), ('r_lambda_factor', C.c_double),
        ('r_lam_exponent', C.c_double),
        ('r_dmin', C.c_double), ('r_dmax', C.c_double), ('s_dmin', C.c_double),
        ('s_dmax', C.c_double),
        ('solid_rule', C.c_int32), ('uniform_grid', C.c_int32),
        ('numeric_intv', C.c_int32), ('tab_degree', C.c_int32),
        ('pad_', C.c_int32), ('table_id', C.c_uint64),
    ]


class SweepParams(C.Structure):
    _fields_ = [
        ('n_rays', C.c_int32), ('n_gates', C.c_int32), ('n_sub', C.c_int32),
        ('n_hnodes', C.c_int32), ('n_vnodes', C.c_int32),
        ('with_melting', C.c_int32), ('with_attenuation', C.c_int32),
        ('integrate_model', C.c_int32), ('apply_sensitivity', C.c_int32),
        ('outputs_on_device', C.c_int32), ('simulate_doppler', C.c_int32),
        ('geometry_mode', C.c_int32),
        ('radar_lat', C.c_double), ('radar_lon', C.c_double), ('radar_alt', C.c_double),
        ('range0', C.c_double), ('range_step', C.c_double),
        ('ke', C.c_double), ('re', C.c_double),
        ('sin_u1', C.c_double), ('cos_u1', C.c_double),
        ('wavelength', C.c_double), ('k_squared', C.c_double), ('radial_res', C.c_double),
        ('c_zh', C.c_double),
        ('var_u', C.c_int32), ('var_v', C.c_int32), ('var_w', C.c_int32), ('var_rho', C.c_int32),
        ('n_vbins', C.c_int32), ('debug_flags', C.c_int32), ('c_spectrum', C.c_double),
        # Doppler scheme 3: spectrum broadening (all zero = off)
        ('turbulence_correction', C.c_int32), ('motion_correction', C.c_int32), ('var_edr', C.c_int32),
        ('terrain_shadow', C.c_int32),              # 1: sub-beams stay blocked behind the topography (cosmo_pol_amd/shadow.py); the former padding
        ('sigma_r', C.c_double), ('sigma_theta', C.c_double), ('motion_num', C.c_double), ('motion_den', C.c_double),
        ('v_res', C.c_double),
    ]


class RayTables(C.Structure):
    _fields_ = [('traj', C.c_void_p), ('geo', C.c_void_p), ('sub_h', C.c_void_p),
                ('sub_v', C.c_void_p), ('sub_w', C.c_void_p), ('sens_thr', C.c_void_p),
                ('site', C.c_void_p), ('paths', C.c_void_p), ('nyquist', C.c_void_p),
                ('version', C.c_uint64), ('varray', C.c_void_p), ('sub_smooth', C.c_void_p),
                ('ml_filter', C.c_void_p),
                ('ml_radius', C.c_int32), ('pad_', C.c_int32),
                # time blend (cpol_run_sweep_members only; all zero = off)
                ('ray_state', C.c_void_p), ('ray_weight', C.c_void_p),
                ('time_blend', C.c_int32), ('pad_time_', C.c_int32)]


OUTPUT_FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V',
                 'RVEL', 'mask', 'species', 'lats', 'lons', 'dist', 'heights', 'visibility', 'model_vars', 'fractions', 'sz_total',
                 'composite', 'histogram', 'DSPECTRUM', 'member_verify', 'mask_sum8', 'spectrum_moments']


SUPEROB_FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'DELTA_HV', 'PHIDP', 'RHOHV', 'ATT_H', 'ATT_V', 'RVEL']    # the rows of `count`


class Superob(C.Structure):
    """cpol_superob: window averages of the per-gate fields (cosmo_pol_amd/superob.py states the rule)."""
    _fields_ = ([('ray_window', C.c_int32), ('gate_window', C.c_int32), ('rays_per_block', C.c_int32), ('pad_', C.c_int32),
                 ('min_valid_fraction', C.c_double)]
                + [(n, C.c_void_p) for n in SUPEROB_FIELDS] + [('count', C.c_void_p)])


MEMBER_STATS_FIELDS = SUPEROB_FIELDS                 # the rows of cpol_member_stats.count
MEMBER_STATS_KINDS = ('mean', 'spread', 'min', 'max')


class MemberStats(C.Structure):
    """cpol_member_stats: the call's member(s) folded into the context's running ensemble statistics
    (cosmo_pol_amd/ensemble_stats.py states the rule).  phase: bit 0 begins a pass, bit 1 finishes it.  The quantile terms
    are appended: a zero-initialised struct has none."""
    _fields_ = ([('phase', C.c_int32), ('min_members', C.c_int32), ('fields', C.c_uint32),
                 ('n_thresholds', C.c_int32 * len(MEMBER_STATS_FIELDS)), ('pad_', C.c_int32),
                 ('thresholds', C.c_void_p * len(MEMBER_STATS_FIELDS))]
                + [(n, C.c_void_p * len(MEMBER_STATS_FIELDS)) for n in MEMBER_STATS_KINDS]
                + [('count', C.c_void_p), ('exceed', C.c_void_p * len(MEMBER_STATS_FIELDS)),
                   ('quantile_capacity', C.c_int32), ('quantile_method', C.c_int32),
                   ('n_quantiles', C.c_int32 * len(MEMBER_STATS_FIELDS)), ('quantiles', C.c_void_p * len(MEMBER_STATS_FIELDS)),
                   ('quantile', C.c_void_p * len(MEMBER_STATS_FIELDS))])


class MemberVerify(C.Structure):
    """cpol_member_verify: the members of a pass of ensemble statistics scored against observations
    (cosmo_pol_amd/ensemble_verify.py states the rule).  fields: bit k = verify field k; a zero-initialised struct verifies
    nothing."""
    _fields_ = ([('fields', C.c_uint32), ('fair', C.c_int32)]
                + [(n, C.c_void_p * len(MEMBER_STATS_FIELDS)) for n in ('obs', 'below', 'equal', 'crps')])


SPECTRUM_MOMENTS_FIELDS = ['POWER', 'VMEAN', 'WIDTH', 'SKEWNESS', 'KURTOSIS', 'VPEAK', 'VLOW', 'VHIGH']    # the rows of `moments`


class SpectrumMoments(C.Structure):
    """cpol_spectrum_moments: the moments of every gate's Doppler spectrum (cosmo_pol_amd/spectrum_moments.py states the
    rule).  fields: bit k = row k of `moments` [8][n_rays * n_gates]."""
    _fields_ = [('fields', C.c_uint32), ('min_bins', C.c_int32), ('min_power', C.c_double), ('moments', C.c_void_p),
                ('count', C.c_void_p)]


SPECIES_FIELDS = ['ZH', 'ZV', 'ZDR', 'KDP', 'RHOHV', 'DELTA_HV', 'ATT_H', 'ATT_V']    # the per-species arrays of a cpol_species


class Species(C.Structure):
    """cpol_species: the radar fields per hydrometeor species, the dominant species and its share (cosmo_pol_amd/species.py
    states the rule).  A NULL array is not written."""
    _fields_ = ([(n, C.c_void_p) for n in SPECIES_FIELDS]
                + [('dominant', C.c_void_p), ('present', C.c_void_p), ('share', C.c_void_p), ('sz', C.c_void_p),
                   ('n_hydro', C.c_int32), ('pad_', C.c_int32)])


HISTOGRAM_FIELDS = SUPEROB_FIELDS                   # the fields of a cpol_histogram: the rows of cpol_superob.count


class Histogram(C.Structure):
    """cpol_histogram: counts of the per-gate fields of a call over many gates (cosmo_pol_amd/histogram.py states the rule)."""
    _fields_ = [('fields', C.c_uint32), ('phase', C.c_int32), ('ordinate', C.c_int32), ('n_y', C.c_int32),
                ('rays_per_block', C.c_int32), ('n_x', C.c_int32 * len(HISTOGRAM_FIELDS)),
                ('edges_x', C.c_void_p * len(HISTOGRAM_FIELDS)), ('edges_y', C.c_void_p),
                ('counts', C.c_void_p * len(HISTOGRAM_FIELDS))]


COMPOSITE_FIELDS = SUPEROB_FIELDS[:9]               # the fields of a cpol_composite: the nine float32 ones


class Composite(C.Structure):
    """cpol_composite: maps of the per-gate fields of a call on a radar-centred grid (cosmo_pol_amd/composite.py states the rule)."""
    _fields_ = [('fields', C.c_uint32), ('phase', C.c_int32), ('products', C.c_uint32), ('rays_per_block', C.c_int32),
                ('n_x', C.c_int32), ('n_y', C.c_int32), ('use_slab', C.c_int32), ('n_thresholds', C.c_int32 * len(COMPOSITE_FIELDS)),
                ('h_lo', C.c_double), ('h_hi', C.c_double), ('thresholds', (C.c_double * 4) * len(COMPOSITE_FIELDS)),
                ('edges_x', C.c_void_p), ('edges_y', C.c_void_p), ('ray_sin', C.c_void_p), ('ray_cos', C.c_void_p),
                ('values', C.c_void_p * len(COMPOSITE_FIELDS)), ('count', C.c_void_p),
                ('plane', C.c_int32), ('source', C.c_int32), ('gate_x', C.c_void_p), ('gate_y', C.c_void_p),
                ('plane_version', C.c_uint64),
                # height layers and the column: a zero-initialised tail means off
                ('n_z', C.c_int32), ('gaps', C.c_int32), ('edges_z', C.c_void_p), ('n_table', C.c_int32 * len(COMPOSITE_FIELDS)),
                ('table_v', C.c_void_p * len(COMPOSITE_FIELDS)), ('table_f', C.c_void_p * len(COMPOSITE_FIELDS)),
                ('column', C.c_void_p * len(COMPOSITE_FIELDS)), ('column_layers', C.c_void_p * len(COMPOSITE_FIELDS))]


class CompositeSums(C.Structure):
    """cpol_composite_sums: a cpol_composite whose products carry CPOL_COMP_SUM, and behind it the weight tables and the outputs
    of the exact sums (composite.py, SUM).  cpol_outputs.composite points at `c`; the library reads beyond it only with the bit."""
    _fields_ = [('c', Composite), ('n_weight', C.c_int32 * len(COMPOSITE_FIELDS)),
                ('weight_v', C.c_void_p * len(COMPOSITE_FIELDS)), ('weight_f', C.c_void_p * len(COMPOSITE_FIELDS)),
                ('sum', C.c_void_p * len(COMPOSITE_FIELDS)), ('sum_skipped', C.c_void_p * len(COMPOSITE_FIELDS))]


OBJ_WORDS = 10                                      # CPOL_OBJ_WORDS: the uint32 words of a row of cpol_objects.table


class Objects(C.Structure):
    """cpol_objects: the object cells of the binary maps of a cpol_fractions (cosmo_pol_amd/objects.py states the rule)."""
    _fields_ = [('connectivity', C.c_int32), ('min_area', C.c_int32), ('max_objects', C.c_int32), ('pad_', C.c_int32),
                ('n_objects', C.c_void_p), ('table', C.c_void_p), ('labels', C.c_void_p),
                # the exact sums: a zero-initialised tail means off
                ('sums', C.c_int32), ('n_weight', C.c_int32), ('weight_v', C.c_void_p), ('weight_f', C.c_void_p),
                ('volume', C.c_void_p), ('skipped', C.c_void_p), ('field', C.c_void_p), ('field_cells', C.c_void_p)]


class ObjectsMatch(C.Structure):
    """cpol_objects_match: a cpol_objects whose pad_ holds max_pieces, and behind it the outputs of the match (objects.py, MATCH).
    cpol_fractions.objects points at `o`; the library reads beyond it only when o.pad_ != 0."""
    _fields_ = [('o', Objects), ('n_pieces', C.c_void_p), ('pieces', C.c_void_p), ('covered', C.c_void_p)]


OBJ_TRACK = 1 << 30                                 # CPOL_OBJ_TRACK in cpol_objects.pad_


class ObjectsTrack(C.Structure):
    """cpol_objects_track: a cpol_objects_match whose o.pad_ carries OBJ_TRACK (its low 16 bits stay max_pieces of the match, 0 =
    that match is off), and behind it the terms and the outputs of the track (objects.py, TRACK).  cpol_fractions.objects points
    at `m.o`; the library reads beyond `m` only with OBJ_TRACK.  shifts_in: a host array."""
    _fields_ = [('m', ObjectsMatch), ('max_shift', C.c_int32), ('max_pieces', C.c_int32), ('shifts_in', C.c_void_p),
                ('correlation', C.c_void_p), ('shift', C.c_void_p), ('n_pieces', C.c_void_p), ('pieces', C.c_void_p),
                ('covered', C.c_void_p)]


class FractionProbabilities(C.Structure):
    """cpol_fraction_probabilities: the neighbourhood ensemble probabilities of the blocks of a cpol_fractions
    (cosmo_pol_amd/neighbourhood.py states the rule: `ensemble_sums`).  member_sum, member_any: NULL = not wanted."""
    _fields_ = [('prob_sums', C.c_void_p), ('reliability', C.c_void_p), ('member_sum', C.c_void_p), ('member_any', C.c_void_p)]


FRAC_PROB_MAX_BLOCKS = 256                          # CPOL_FRAC_PROB_MAX_BLOCKS


class Fractions(C.Structure):
    """cpol_fractions: the fractions skill score's sums of one finished plane of a composite against an observed map
    (cosmo_pol_amd/neighbourhood.py states the rule).  objects: NULL (a zero-initialised struct) = no object cells."""
    _fields_ = [('field', C.c_int32), ('plane', C.c_int32), ('n_thresholds', C.c_int32), ('n_radii', C.c_int32),
                ('thresholds', C.c_double * 4), ('radii', C.c_int32 * 8), ('observed', C.c_void_p), ('domain', C.c_void_p),
                ('sums', C.c_void_p), ('totals', C.c_void_p), ('objects', C.POINTER(Objects))]


FRAC_ENSEMBLE = 0x10000                             # CPOL_FRAC_ENSEMBLE, or-ed into Fractions.n_radii


class FractionsEnsemble(C.Structure):
    """cpol_fractions_ensemble: a cpol_fractions whose n_radii carries CPOL_FRAC_ENSEMBLE, and behind it the pointer to the
    neighbourhood ensemble probabilities.  cpol_outputs.fractions points at `f`; the library reads beyond it only with the flag."""
    _fields_ = [('f', Fractions), ('probabilities', C.POINTER(FractionProbabilities))]


class _ObjectsNamed(object):
    """What objects.result reads of a spec, for the test hook: the cells' terms and the thresholds as the library rounds them."""

    def __init__(self, objects, spec, grid):
        self.connectivity, self.min_area = objects.connectivity, objects.min_area
        self.weight, (self.n_y, self.n_x) = getattr(objects, 'weight', None), grid
        with np.errstate(over='ignore'):
            self.thresholds = np.array(spec.thresholds_given, dtype=np.float64).astype(np.float32)


class Outputs(C.Structure):
    # species (directly behind mask, in front of every member that is pinned where it is), spectrum_moments (the last of OUTPUT_FIELDS), member_verify (directly before mask_sum8), histogram (directly before DSPECTRUM), composite (directly before histogram) and fractions (directly before sz_total, in front of the members that are pinned where they are): pointers to a struct, not
    # arrays; member_stats, superob likewise: NULL = off; superob stays the last member (cpol_outputs)
    _fields_ = ([(n, {'species': C.POINTER(Species), 'spectrum_moments': C.POINTER(SpectrumMoments), 'member_verify': C.POINTER(MemberVerify),
                      'histogram': C.POINTER(Histogram), 'composite': C.POINTER(Composite),
                      'fractions': C.POINTER(Fractions)}.get(n, C.c_void_p))
                 for n in OUTPUT_FIELDS]
                + [('member_stats', C.POINTER(MemberStats)), ('superob', C.POINTER(Superob))])


class SubbeamOutputs(C.Structure):
    """cpol_subbeam_outputs: the sub-beam columns of cpol_interp_subbeams."""
    _fields_ = [('vals', C.c_void_p), ('mask', C.c_void_p), ('elev', C.c_void_p), ('lats', C.c_void_p),
                ('lons', C.c_void_p), ('dist', C.c_void_p), ('heights', C.c_void_p), ('q_melt', C.c_void_p),
                ('fw_melt', C.c_void_p), ('mask_ml', C.c_void_p), ('wgate', C.c_void_p),
                ('skip_melting', C.c_int32), ('outputs_on_device', C.c_int32)]


class Columns(C.Structure):
    """cpol_columns_t: caller-supplied sub-beam columns of cpol_run_columns."""
    _fields_ = [('n_vars', C.c_int32), ('inputs_on_device', C.c_int32), ('vals', C.c_void_p),
                ('mask', C.c_void_p), ('elev', C.c_void_p), ('wgate', C.c_void_p), ('q_melt', C.c_void_p),
                ('fw_melt', C.c_void_p), ('has_melting', C.c_void_p), ('az_sincos', C.c_void_p),
                ('sub_w', C.c_void_p), ('nyquist', C.c_void_p), ('sens_thr', C.c_void_p), ('varray', C.c_void_p)]


class Counters(C.Structure):
    _fields_ = [('n_subbeam_gates', C.c_int64), ('n_valid_items', C.c_int64),
                ('n_gates', C.c_int64), ('n_work_units', C.c_int64),
                ('ms_traj', C.c_float), ('ms_interp', C.c_float), ('ms_classify', C.c_float),
                ('ms_bucket', C.c_float), ('ms_psd', C.c_float), ('ms_final', C.c_float),
                ('ms_total', C.c_float), ('n_table_items', C.c_int32), ('pad_', C.c_int32)]


MAX_VARS, MAX_RAW_FIELDS, MAX_LOAD = 24, 32, 8          # CPOL_MAX_VARS / CPOL_MAX_RAW_FIELDS / CPOL_MAX_LOAD
RECIPE_COPY, RECIPE_HALF_MEAN, RECIPE_RHO, RECIPE_TIMES_RHO, RECIPE_ZEROS = range(5)


class PackedPlane(C.Structure):
    """cpol_packed_plane: one GRIB-1 message's bit string and scale factors."""
    _fields_ = [('octets', C.c_void_p), ('n_octets', C.c_int64), ('ref_value', C.c_double), ('bin_scale', C.c_int32),
                ('dec_scale', C.c_int32), ('n_bits', C.c_int32), ('flip_rows', C.c_int32), ('field', C.c_int32),
                ('level', C.c_int32)]


class PackedModel(C.Structure):
    """cpol_packed_model: the raw fields of the planes and the recipe of every staged variable."""
    _fields_ = [('nz', C.c_int32), ('ny', C.c_int32), ('nx', C.c_int32), ('n_fields', C.c_int32),
                ('field_levels', C.c_int32 * MAX_RAW_FIELDS), ('field_p', C.c_int32), ('field_t', C.c_int32),
                ('field_qv', C.c_int32), ('field_hhl', C.c_int32), ('n_load', C.c_int32),
                ('field_load', C.c_int32 * MAX_LOAD), ('n_vars', C.c_int32), ('recipe', C.c_int32 * MAX_VARS),
                ('source', C.c_int32 * MAX_VARS), ('r_d', C.c_double), ('rv_rd_m1', C.c_double),
                ('llc', C.c_float * 2), ('urc', C.c_float * 2), ('res', C.c_float * 2), ('south_pole', C.c_double * 2)]


EXPORTS = ['cpol_create', 'cpol_destroy', 'cpol_fork', 'cpol_last_error', 'cpol_set_stream',
           'cpol_get_stream',
           'cpol_synchronize', 'cpol_stage_model', 'cpol_stage_hydro', 'cpol_set_num_hydro',
           'cpol_stage_doppler_weights', 'cpol_stage_spectrum_tables', 'cpol_stage_t_function', 'cpol_prepare',
           'cpol_interp_points', 'cpol_ray_tables', 'cpol_run_sweep', 'cpol_interp_subbeams', 'cpol_run_columns', 'cpol_counters',
           'cpol_spaceborne_first_gate', 'cpol_host_alloc', 'cpol_host_free', 'cpol_host_alloc_near',
           'cpol_device_pci_bus_id', 'cpol_mem_info',
           'cpol_enable_timing', 'cpol_debug_read', 'cpol_debug_math', 'cpol_debug_scan', 'cpol_broaden_rows',
           'cpol_stage_model_packed', 'cpol_unpack_planes',
           'cpol_stage_member', 'cpol_num_members', 'cpol_select_member', 'cpol_run_sweep_members']
MEMBERS_PER_CALL = 64                               # members one cpol_run_sweep_members call takes

TRAJ_STRIDE, GEO_STRIDE, SITE_STRIDE = 4, 8, 8      # CPOL_*_STRIDE of the header
MELT_DEGREE, MELT_FUNCS = 10, 4                    # CPOL_MELT_DEGREE / CPOL_MELT_FUNCS
ICE_DEGREE, ICE_FUNCS = 10, 3                      # CPOL_ICE_DEGREE / CPOL_ICE_FUNCS
TFUN_SNOW_N0, TFUN_ICE_MOM2_A = 0, 1
TFUN_FIRST_BITS, TFUN_COUNT = 0x43000000, 1 << 24  # every float32 in [128, 512)

_lib = None
_torch_hip = None


class NativeError(RuntimeError):
    pass


def hip_runtimes_mapped():
    """Distinct libamdhip64 files mapped into this process (/proc/self/maps)."""
    found = []
    try:
        with open('/proc/self/maps') as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                if 'libamdhip64' in os.path.basename(path):
                    real = os.path.realpath(path)
                    if real not in found:
                        found.append(real)
    except OSError:
        pass
    return found


def _share_torch_hip_runtime():
    """One HIP runtime per process.  libcosmo_pol_hip.so needs `libamdhip64.so.7`; a PyTorch-ROCm
    wheel bundles its own copy of that runtime (same SONAME) and asks for it as `libamdhip64.so`.
    If this library comes first the loader serves it from /opt/rocm and torch later maps its
    bundled copy as well: two runtimes, and the second one to initialise finds no GPU
    ("No HIP GPUs are available" in torch._C._cuda_init).  So when a torch wheel with a bundled
    runtime is installed -- found without importing torch -- that copy is mapped first; this
    library then binds to it by SONAME and a later `import torch` finds it already loaded.
    CPOL_HIP_RUNTIME=system skips this (a process that will never touch torch.cuda)."""
    import sys
    if os.environ.get('CPOL_HIP_RUNTIME', '') == 'system' or hip_runtimes_mapped():
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if not os.path.exists(cand):
        return None
    try:
        return C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError as e:
        print('cosmo_pol_amd: could not preload %s (%s); using the system HIP runtime' % (cand, e),
              file=sys.stderr)
        return None


def load_library():
    """Loads the HIP shared library (never falls back to anything else)."""
    global _lib, _torch_hip
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            'cosmo_pol_amd: HIP extension %s is missing. Build it with '
            '`python -c "import __graft_entry__ as g; g.build()"` or `make -C cosmo_pol_amd/csrc`. '
            'There is no CPU fallback.' % LIB_PATH)
    _torch_hip = _share_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    if len(hip_runtimes_mapped()) > 1:
        raise NativeError(
            'cosmo_pol_amd: two HIP runtimes are mapped into this process (%s): the second one to '
            'initialise will not see the GPU.  Import cosmo_pol_amd (or torch) before any other '
            'package that loads libamdhip64, or unset CPOL_HIP_RUNTIME.' % ', '.join(hip_runtimes_mapped()))
    vp = C.c_void_p
    lib.cpol_create.restype = C.c_int
    lib.cpol_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.cpol_get_stream.restype = C.c_int
    lib.cpol_get_stream.argtypes = [vp, C.POINTER(vp)]
    lib.cpol_fork.restype = C.c_int
    lib.cpol_fork.argtypes = [vp, C.POINTER(vp)]
    lib.cpol_destroy.restype = None
    lib.cpol_destroy.argtypes = [vp]
    lib.cpol_last_error.restype = C.c_char_p
    lib.cpol_last_error.argtypes = [vp]
    lib.cpol_set_stream.restype = C.c_int
    lib.cpol_set_stream.argtypes = [vp, vp]
    lib.cpol_synchronize.restype = C.c_int
    lib.cpol_synchronize.argtypes = [vp]
    lib.cpol_stage_model.restype = C.c_int
    lib.cpol_stage_model.argtypes = [vp, C.c_int, C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int,
                                     vp, vp, vp, vp]
    lib.cpol_stage_model_packed.restype = C.c_int
    lib.cpol_stage_model_packed.argtypes = [vp, C.POINTER(PackedModel), C.POINTER(PackedPlane), C.c_int]
    lib.cpol_unpack_planes.restype = C.c_int
    lib.cpol_unpack_planes.argtypes = [vp, C.POINTER(PackedPlane), C.c_int, C.c_int, C.c_int, vp]
    lib.cpol_stage_hydro.restype = C.c_int
    lib.cpol_stage_hydro.argtypes = [vp, C.c_int, C.POINTER(HydroDesc), vp, vp, vp, vp, C.c_int]
    lib.cpol_stage_doppler_weights.restype = C.c_int
    lib.cpol_stage_doppler_weights.argtypes = [vp, C.c_int, vp]
    lib.cpol_set_num_hydro.restype = C.c_int
    lib.cpol_set_num_hydro.argtypes = [vp, C.c_int]
    lib.cpol_interp_points.restype = C.c_int
    lib.cpol_interp_points.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.cpol_broaden_rows.restype = C.c_int
    lib.cpol_broaden_rows.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.cpol_ray_tables.restype = C.c_int
    lib.cpol_ray_tables.argtypes = [C.POINTER(SweepParams), vp, vp, vp, vp, vp, vp]
    lib.cpol_run_sweep.restype = C.c_int
    lib.cpol_run_sweep.argtypes = [vp, C.POINTER(SweepParams), C.POINTER(RayTables),
                                   C.POINTER(Outputs)]
    lib.cpol_interp_subbeams.restype = C.c_int
    lib.cpol_interp_subbeams.argtypes = [vp, C.POINTER(SweepParams), C.POINTER(RayTables), C.POINTER(SubbeamOutputs)]
    lib.cpol_run_columns.restype = C.c_int
    lib.cpol_run_columns.argtypes = [vp, C.POINTER(SweepParams), C.POINTER(Columns), C.POINTER(Outputs)]
    lib.cpol_counters.restype = C.c_int
    lib.cpol_counters.argtypes = [vp, C.POINTER(Counters)]
    lib.cpol_spaceborne_first_gate.restype = C.c_int
    lib.cpol_spaceborne_first_gate.argtypes = [vp, C.POINTER(SweepParams), vp, vp, vp, C.c_double, vp]
    lib.cpol_enable_timing.restype = C.c_int
    lib.cpol_enable_timing.argtypes = [vp, C.c_int]
    lib.cpol_debug_read.restype = C.c_int64
    lib.cpol_debug_read.argtypes = [vp, C.c_char_p, vp, C.c_int64]
    lib.cpol_stage_spectrum_tables.restype = C.c_int
    lib.cpol_stage_spectrum_tables.argtypes = [vp, C.c_int, vp, vp]
    lib.cpol_debug_math.restype = C.c_int
    lib.cpol_debug_math.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    lib.cpol_debug_scan.restype = C.c_int
    lib.cpol_debug_scan.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int]
    lib.cpol_prepare.restype = C.c_int
    lib.cpol_prepare.argtypes = [vp]
    lib.cpol_stage_t_function.restype = C.c_int
    lib.cpol_stage_t_function.argtypes = [vp, C.c_int, vp]
    lib.cpol_host_alloc.restype = C.c_int
    lib.cpol_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]      # (ctx may be NULL: context-free block)
    lib.cpol_host_free.restype = C.c_int
    lib.cpol_host_free.argtypes = [vp, vp]
    lib.cpol_host_alloc_near.restype = C.c_int
    lib.cpol_host_alloc_near.argtypes = [C.c_int, C.c_size_t, C.POINTER(vp)]
    lib.cpol_mem_info.restype = C.c_int
    lib.cpol_mem_info.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.cpol_stage_member.restype = C.c_int
    lib.cpol_stage_member.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.cpol_num_members.restype = C.c_int
    lib.cpol_num_members.argtypes = [vp]
    lib.cpol_select_member.restype = C.c_int
    lib.cpol_select_member.argtypes = [vp, C.c_int]
    lib.cpol_run_sweep_members.restype = C.c_int
    lib.cpol_run_sweep_members.argtypes = [vp, C.POINTER(SweepParams), C.POINTER(RayTables), vp, C.c_int, C.POINTER(Outputs)]
    lib.cpol_device_pci_bus_id.restype = C.c_int
    lib.cpol_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    _lib = lib
    return lib


def parse_cpulist(text):
    """'0-3,8,10-11' (sysfs cpulist) -> set of ints."""
    cpus = set()
    for part in text.strip().split(','):
        if not part:
            continue
        lo, _, hi = part.partition('-')
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def device_numa_info(device=0, sysfs='/sys/bus/pci/devices', pci=None):
    """{'pci': '0000:75:00.0', 'node': 1, 'cpus': {...}} of GPU `device` (HIP ordinal); node / cpus are
    None / empty where the kernel does not tell (one-socket hosts report node -1).  `pci`: the bus id
    when it is known already (tests)."""
    if pci is None:
        lib = load_library()
        buf = C.create_string_buffer(64)
        if lib.cpol_device_pci_bus_id(int(device), buf, 64) != 0:
            raise NativeError('cpol_device_pci_bus_id(%d) failed: no such GPU' % device)
        pci = buf.value.decode()
    bdf = pci.lower()
    info = {'pci': bdf, 'node': None, 'cpus': set()}
    try:
        with open(os.path.join(sysfs, bdf, 'numa_node')) as f:
            node = int(f.read().strip())
        info['node'] = node if node >= 0 else None
        with open(os.path.join(sysfs, bdf, 'local_cpulist')) as f:
            info['cpus'] = parse_cpulist(f.read())
    except (OSError, ValueError):
        pass
    return info


def bind_to_device_numa_node(device=0, sysfs='/sys/bus/pci/devices', pci=None):
    """One process per GPU on a multi-socket host: restricts the calling thread (and every thread it
    starts afterwards) to the cores next to GPU `device`, so that the threads which build ray tables,
    fill upload buffers and read results run on the socket whose memory the GPU's copies land in
    (PinnedPool takes its blocks there, cpol_host_alloc_near).  Call it before the operator creates its
    lane threads.  Never widens the affinity the process was given; does nothing when the GPU's cores
    and the allowed cores do not intersect or the kernel reports no node.  CPOL_NUMA_BIND=0 switches
    it off.  -> the info dict of device_numa_info plus 'bound' (number of cores, 0 = unchanged)."""
    info = device_numa_info(device, sysfs, pci)
    info['bound'] = 0
    if os.environ.get('CPOL_NUMA_BIND', '1') == '0' or not info['cpus'] or not hasattr(os, 'sched_setaffinity'):
        return info
    allowed = os.sched_getaffinity(0)
    want = allowed & info['cpus']
    if want and want != allowed:
        os.sched_setaffinity(0, want)
        info['bound'] = len(want)
    return info


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class PinnedPool(object):
    """Page-locked host blocks for results handed to the user.

    `take(nbytes)` returns a uint8 ndarray over a block of context-free pinned memory
    (cpol_host_alloc(NULL, ...)).  The block belongs to that array and to every view carved from it:
    when the last of them is garbage-collected the block goes back to the pool and is re-used by a
    later `take` of the same size class -- so results stay valid for as long as anybody holds them,
    whatever happens to the operator, its lanes or its contexts in the meantime, and a steady stream
    of equal sweeps allocates nothing.  A block that was the target of a non-blocking device-to-host
    copy remembers the context that issued it (`pending`); re-use waits for that context first."""
    GRANULE = 1 << 20
    MAX_PENDING = 8             # blocks of one size class that may wait for foreign copies before the pool waits

    def __init__(self, device=None):
        import collections
        import threading
        self.lib = load_library()
        self.device = device        # blocks come from the NUMA node next to this GPU (None: the current device's)
        self.free = {}              # size class -> [(address, context or None, serial)]
        self.returned = collections.deque()     # blocks handed back by finalizers, not yet sorted into `free`
        self.lock = threading.Lock()
        self.closed = False
        self.n_alloc = 0

    def _release(self, addr, size, holder):
        # Runs as a weakref finalizer: on ANY thread, possibly inside a garbage collection triggered by an
        # allocation made while that thread holds self.lock (a result kept alive only by a reference cycle).
        # So it never takes the lock: deque.append / popleft are atomic, take() sorts the blocks in.
        self.returned.append((addr, size, holder.get('ctx'), holder.get('serial', 0)))
        if self.closed:
            self._free_returned()

    def _free_returned(self):
        while True:
            try:
                addr = self.returned.popleft()[0]
            except IndexError:
                return
            self.lib.cpol_host_free(None, C.c_void_p(addr))

    @staticmethod
    def _clean(ctx, serial):
        """No copy into the block can still be in flight."""
        return ctx is None or not getattr(ctx, 'h', None) or ctx.completed >= serial

    def take(self, nbytes, writer=None):
        """-> (uint8 array over a block of >= nbytes, holder).  `writer`: the context whose stream
        will copy into the block.  A block whose last copy (queued by context C, not yet waited for)
        may still be in flight is handed out again without waiting only to C itself -- copies on one
        stream stay in order, and nobody holds the old arrays any more; for another writer the pool
        prefers a clean block, then a new one (up to MAX_PENDING blocks in flight), then waits for C.
        After queueing a non-blocking copy set holder['ctx'], holder['serial'] = context, its
        `submitted` count."""
        import weakref
        size = max(1, -(-int(nbytes) // self.GRANULE)) * self.GRANULE
        addr = wait_for = None
        with self.lock:
            while True:                                                   # blocks handed back since the last call
                try:
                    a, sz, c, ser = self.returned.popleft()
                except IndexError:
                    break
                self.free.setdefault(sz, []).append((a, c, ser))
            lst = self.free.get(size) or []
            pick = None
            for i, (a, c, ser) in enumerate(lst):                    # oldest first
                if c is writer or self._clean(c, ser):
                    pick = i
                    break
            if pick is None and lst and len(lst) >= self.MAX_PENDING:
                pick = 0
                wait_for = lst[0][1]
            if pick is not None:
                addr = lst.pop(pick)[0]
        if wait_for is not None:
            wait_for.synchronize()  # (also surfaces a deferred domain error of that lane, once)
        if addr is None:
            h = C.c_void_p()
            if self.device is None:
                rc = self.lib.cpol_host_alloc(None, size, C.byref(h))
            else:
                rc = self.lib.cpol_host_alloc_near(int(self.device), size, C.byref(h))
            if rc != 0 or not h:
                raise MemoryError('cpol_host_alloc(%d bytes of page-locked host memory) failed' % size)
            addr = h.value
            self.n_alloc += 1
        buf = (C.c_uint8 * size).from_address(addr)
        arr = np.frombuffer(buf, dtype=np.uint8)
        holder = {'ctx': None, 'serial': 0}
        weakref.finalize(arr, self._release, addr, size, holder)
        return arr, holder

    def close(self):
        """Frees the blocks nobody holds; blocks still held are freed when their last view dies."""
        with self.lock:
            self.closed = True
            blocks = [e[0] for lst in self.free.values() for e in lst]
            self.free = {}
        for a in blocks:
            self.lib.cpol_host_free(None, C.c_void_p(a))
        self._free_returned()


_ITEMSIZE = {np.float32: 4, np.float64: 8, np.int8: 1, np.uint8: 1, np.uint16: 2, np.uint64: 8, np.uint32: 4, np.int32: 4}


def carve_block(pool, spec, writer=None):
    """`spec` [(key, dtype, shape), ...] -> (views, addresses, holder): one block of `pool` (`take`) cut into 64-byte
    aligned arrays, in the order of `spec`.  Every host output of a call is such a view: the kernels write a device image
    of the block and a single device-to-host copy, queued behind them, moves it.  The block belongs to the arrays: it
    returns to the pool when the last of them is dropped, whatever happens to the lanes or the operator in between."""
    counts = [math.prod(sh) for _, _, sh in spec]
    sizes = [-(-n_el * _ITEMSIZE[dt] // 64) * 64 for n_el, (_, dt, _) in zip(counts, spec)]
    slab, holder = pool.take(sum(sizes), writer=writer)
    base = slab.ctypes.data               # (base + off = the view's .ctypes.data, without an interface object per array)
    views, addresses, off = [], [], 0
    for (_, dt, sh), n_el, nb in zip(spec, counts, sizes):
        views.append(slab[off:off + n_el * _ITEMSIZE[dt]].view(dt).reshape(sh))
        addresses.append(base + off)
        off += nb
    return views, addresses, holder


class Context(object):
    """One device context (one per GPU per process)."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.cpol_create(int(device), C.byref(h))
        if rc != 0 or not h:
            raise NativeError('cpol_create(device=%d) failed with status %d (no usable HIP '
                              'device?)' % (device, rc))
        self.h = h
        self.device = device
        self.n_vars = 0
        self._keep = []
        self.submitted = self.completed = 0     # sweeps queued / known to have completed (synchronize)

    def fork(self):
        """A lane: shares this context's staged model / tables, own stream and work
        buffers (cpol_fork).  Close lanes before their parent."""
        h = C.c_void_p()
        self._check(self.lib.cpol_fork(self.h, C.byref(h)), 'cpol_fork')
        lane = Context.__new__(Context)
        lane.lib, lane.h, lane.device, lane.n_vars = self.lib, h, self.device, self.n_vars
        lane._keep = []
        lane.submitted = lane.completed = 0
        lane._parent = self          # keeps the parent alive
        return lane

    def close(self):
        if getattr(self, 'h', None):
            self.lib.cpol_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc == 0:
            return
        msg = self.lib.cpol_last_error(self.h)
        msg = msg.decode() if msg else ''
        if rc == ERR_DOMAIN:
            raise IndexError('ERROR: ' + msg + ': ABORTING')
        if rc == ERR_ARG:
            raise ValueError('%s: %s' % (what, msg))
        if rc == ERR_NOMEM:
            raise MemoryError('%s: %s' % (what, msg))
        raise NativeError('%s failed (%d): %s' % (what, rc, msg))

    def set_stream(self, stream_ptr):
        self._check(self.lib.cpol_set_stream(self.h, C.c_void_p(stream_ptr)), 'cpol_set_stream')

    def synchronize(self):
        """Waits for the context's stream; raises IndexError if a sweep since the last
        report left the model domain (deferred error of device / pinned-host outputs)."""
        n = self.submitted
        rc = self.lib.cpol_synchronize(self.h)
        self.completed = max(self.completed, n)          # (the stream has drained, error or not)
        self._check(rc, 'cpol_synchronize')

    def host_alloc(self, nbytes):
        """uint8 array over page-locked host memory owned by the context (the target of
        outputs_on_device = 2); valid until the context is closed."""
        h = C.c_void_p()
        self._check(self.lib.cpol_host_alloc(self.h, int(nbytes), C.byref(h)), 'cpol_host_alloc')
        buf = (C.c_uint8 * int(nbytes)).from_address(h.value)
        arr = np.frombuffer(buf, dtype=np.uint8)
        self._keep.append(buf)
        return arr

    def mem_info(self):
        """(free bytes, total bytes) of the GPU's memory, work-buffer bytes per sub-beam gate of a launch sequence."""
        f, t, g = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self.lib.cpol_mem_info(self.h, C.byref(f), C.byref(t), C.byref(g)), 'cpol_mem_info')
        return int(f.value), int(t.value), int(g.value)

    def enable_timing(self, on=True):
        """True / 1: events around every stage; 2: around the PSD stage only; False: off."""
        self._check(self.lib.cpol_enable_timing(self.h, 2 if on == 2 else int(bool(on))),
                    'cpol_enable_timing')

    def stream_ptr(self):
        h = C.c_void_p()
        self._check(self.lib.cpol_get_stream(self.h, C.byref(h)), 'cpol_get_stream')
        return h.value or 0

    def enable_debug(self, on=True):
        self.lib.cpol_debug_read(self.h, b'enable' if on else b'disable', None, 0)

    def set_stencil_budget(self, nbytes):
        """Bytes of device memory the gate stencils of this (root) context may hold; 0 turns them off.  Refused (ValueError) while
        lanes of the context exist; lowering it below what is held drops every stencil.  (cpol_debug_read "stencil_budget".)"""
        v = C.c_uint64(int(nbytes))
        self._check(int(self.lib.cpol_debug_read(self.h, b'stencil_budget', C.byref(v), 8)), 'cpol_debug_read(stencil_budget)')

    def stencil_state(self):
        """{'form': of this context's last sweep (0 full, 1 recording, 2 replay), and of the root's store: 'entries', 'bytes',
        'records', 'replays', 'drops'} (cpol_debug_read "stencil")."""
        out = np.zeros(6, dtype=np.float64)
        n = self.lib.cpol_debug_read(self.h, b'stencil', _ptr(out), out.nbytes)
        if n != out.nbytes:
            self._check(int(n) if n < 0 else ERR_ARG, 'cpol_debug_read(stencil)')
        return dict(zip(('form', 'entries', 'bytes', 'records', 'replays', 'drops'), (int(x) for x in out)))

    def stage_model(self, arrays, zlevels, llc, urc, res, south_pole):
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        zlevels = np.ascontiguousarray(zlevels, dtype=np.float32)
        nz, ny, nx = zlevels.shape
        for a in arrays:
            if a.shape != (nz, ny, nx):
                raise ValueError('model variable shape %s != z-levels shape %s'
                                 % (a.shape, zlevels.shape))
        ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        llc = np.ascontiguousarray(llc, dtype=np.float32)
        urc = np.ascontiguousarray(urc, dtype=np.float32)
        res = np.ascontiguousarray(res, dtype=np.float32)
        sp = np.ascontiguousarray(south_pole, dtype=np.float64)
        rc = self.lib.cpol_stage_model(self.h, len(arrays), ptrs, _ptr(zlevels), nz, ny, nx,
                                       _ptr(llc), _ptr(urc), _ptr(res), _ptr(sp))
        self._check(rc, 'cpol_stage_model')
        self.n_vars = len(arrays)
        self.model_shape = (nz, ny, nx)

    def stage_member(self, member, arrays):
        """The variables of ensemble member `member` (same order and [nz, ny, nx] shape as the staged cube, which is member 0)."""
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        want = getattr(self, 'model_shape', None)
        if want is None or len(arrays) != getattr(self, 'n_vars', -1):
            raise ValueError('stage_member: needs a staged model with the same number of variables')
        for a in arrays:
            if a.shape != want:            # (the library reads nz * ny * nx values from every pointer)
                raise ValueError('member variable shape %s != staged cube shape %s' % (a.shape, want))
        ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        self._check(self.lib.cpol_stage_member(self.h, int(member), len(arrays), ptrs), 'cpol_stage_member')

    def num_members(self):
        return int(self.lib.cpol_num_members(self.h))

    def select_member(self, member):
        self._check(self.lib.cpol_select_member(self.h, int(member)), 'cpol_select_member')

    def run_sweep_members(self, params, tables, members, outputs):
        members = np.ascontiguousarray(members, dtype=np.int32)
        self.submitted += 1
        rc = self.lib.cpol_run_sweep_members(self.h, C.byref(params), C.byref(tables), _ptr(members), len(members),
                                             C.byref(outputs))
        self._check(rc, 'cpol_run_sweep_members')

    @staticmethod
    def packed_planes(planes):
        """[(octets: uint8 array, R, E, D, n_bits, flip, field, level)] -> (PackedPlane array, what keeps the octets alive)."""
        arr = (PackedPlane * len(planes))()
        keep = []
        for d, (octets, R, E, D, n_bits, flip, field, level) in zip(arr, planes):
            octets = np.ascontiguousarray(octets, dtype=np.uint8)
            keep.append(octets)
            d.octets, d.n_octets = (octets.ctypes.data if octets.size else None), octets.size
            d.ref_value, d.bin_scale, d.dec_scale, d.n_bits = float(R), int(E), int(D), int(n_bits)
            d.flip_rows, d.field, d.level = int(bool(flip)), int(field), int(level)
        return arr, keep

    def unpack_planes(self, planes, ny, nx):
        """k_grib_unpack on caller planes (see packed_planes; field / level unused) -> float32 [n, ny, nx]."""
        arr, keep = self.packed_planes(planes)
        out = np.empty((len(planes), ny, nx), dtype=np.float32)
        rc = self.lib.cpol_unpack_planes(self.h, arr, len(planes), int(ny), int(nx), _ptr(out))
        self._check(rc, 'cpol_unpack_planes')
        return out

    def stage_model_packed(self, model, planes):
        """model: PackedModel; planes as for packed_planes.  Unpacks, derives and stages on the device."""
        arr, keep = self.packed_planes(planes)
        rc = self.lib.cpol_stage_model_packed(self.h, C.byref(model), arr, len(planes))
        self._check(rc, 'cpol_stage_model_packed')
        self.n_vars = int(model.n_vars)
        self.model_shape = (int(model.nz), int(model.ny), int(model.nx))

    def ingest_times(self):
        """Milliseconds of the last stage_model_packed: octets to the device, k_grib_unpack, k_model_derive, the whole call."""
        v = self.debug_read('ingest_times', (4,), np.float64)
        return {'upload_ms': v[0], 'unpack_ms': v[1], 'derive_ms': v[2], 'total_ms': v[3]}

    def stage_hydro(self, slot, desc, table, pre=None, dnu=None, aux=None):
        table = np.ascontiguousarray(table, dtype=np.float64)
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        pre, dnu, aux = f64(pre), f64(dnu), f64(aux)
        rc = self.lib.cpol_stage_hydro(self.h, slot, C.byref(desc), _ptr(table), _ptr(pre),
                                       _ptr(dnu), _ptr(aux), 0 if aux is None else aux.size)
        self._check(rc, 'cpol_stage_hydro')

    def stage_doppler_weights(self, slot, weights):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        self._check(self.lib.cpol_stage_doppler_weights(self.h, slot, _ptr(w)),
                    'cpol_stage_doppler_weights')

    def stage_spectrum_tables(self, slot, rcs32, dgrid):
        rcs32 = np.ascontiguousarray(rcs32, dtype=np.float32)
        dgrid = np.ascontiguousarray(dgrid, dtype=np.float32)
        self._check(self.lib.cpol_stage_spectrum_tables(self.h, int(slot), _ptr(rcs32), _ptr(dgrid)),
                    'cpol_stage_spectrum_tables')

    def stage_t_function(self, which, table):
        table = np.ascontiguousarray(table, dtype=np.float32)
        if table.size != TFUN_COUNT:
            raise ValueError('t-function table must have %d entries' % TFUN_COUNT)
        self._check(self.lib.cpol_stage_t_function(self.h, int(which), _ptr(table)),
                    'cpol_stage_t_function')

    def prepare(self):
        """Builds the integral tables now (otherwise: at the first sweep / fork)."""
        self._check(self.lib.cpol_prepare(self.h), 'cpol_prepare')

    def set_num_hydro(self, n):
        self._check(self.lib.cpol_set_num_hydro(self.h, n), 'cpol_set_num_hydro')

    def interp_points(self, coords, heights):
        coords = np.ascontiguousarray(coords, dtype=np.float32)
        heights = np.ascontiguousarray(heights, dtype=np.float32)
        n = heights.shape[0]
        out = np.empty((self.n_vars, n), dtype=np.float32)
        rc = self.lib.cpol_interp_points(self.h, n, _ptr(coords), _ptr(heights), _ptr(out))
        self._check(rc, 'cpol_interp_points')
        return out

    def broaden_rows(self, rows, sigma_bins):
        """The filter of the spectrum broadening on explicit float32 rows [n_rows, n_v], one sigma in bins per row."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        sigma_bins = np.ascontiguousarray(sigma_bins, dtype=np.float64)
        if rows.ndim != 2 or sigma_bins.shape != (rows.shape[0],):
            raise ValueError('broaden_rows: rows [n_rows, n_v] and one sigma per row')
        out = np.empty_like(rows)
        rc = self.lib.cpol_broaden_rows(self.h, _ptr(rows), rows.shape[0], rows.shape[1], _ptr(sigma_bins), _ptr(out))
        self._check(rc, 'cpol_broaden_rows')
        return out

    def run_sweep(self, params, tables, outputs):
        self.submitted += 1
        rc = self.lib.cpol_run_sweep(self.h, C.byref(params), C.byref(tables), C.byref(outputs))
        self._check(rc, 'cpol_run_sweep')

    def interp_subbeams(self, params, tables, outputs):
        self.submitted += 1
        rc = self.lib.cpol_interp_subbeams(self.h, C.byref(params), C.byref(tables), C.byref(outputs))
        self._check(rc, 'cpol_interp_subbeams')

    def run_columns(self, params, columns, outputs):
        self.submitted += 1
        rc = self.lib.cpol_run_columns(self.h, C.byref(params), C.byref(columns), C.byref(outputs))
        self._check(rc, 'cpol_run_columns')

    def spaceborne_first_gate(self, params, traj, site, n_cand, ceiling_m):
        n = params.n_rays * params.n_vnodes
        out = np.empty(n, dtype=np.int32)
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        site = np.ascontiguousarray(site, dtype=np.float64)
        n_cand = np.ascontiguousarray(n_cand, dtype=np.int32)
        rc = self.lib.cpol_spaceborne_first_gate(self.h, C.byref(params), _ptr(traj), _ptr(site),
                                                 _ptr(n_cand), float(ceiling_m), _ptr(out))
        self._check(rc, 'cpol_spaceborne_first_gate')
        return out.reshape(params.n_rays, params.n_vnodes)

    def counters(self):
        c = Counters()
        self._check(self.lib.cpol_counters(self.h, C.byref(c)), 'cpol_counters')
        return c

    def itab_report(self):
        """Accuracy gate of the integral tables of the staged slots (cpol_prepare): per slot the worst
        deviation of a block's polynomial from the integrating kernel at the block's check point
        (`check`: negative = table rejected, the slot is integrated bin by bin; 0 = no table), where it
        was found (`at`), the number of (block, function) pairs above the limit (`n_bad`, 1-D tables),
        the worst deviation at the second check point alone -- u = 0.96, between the last two nodes of a
        lambda panel (`check_edge`, 1-D tables; `check` is the maximum over both points) -- and the device
        time of the build and of the check alone (`build_ms`, `check_ms`)."""
        a = self.debug_read('itab_check', (4, CPOL_MAX_HYDRO), np.float64)
        t = self.debug_read('itab_times', (CPOL_MAX_HYDRO, 2), np.float64)
        return {'check': a[0], 'at': a[1], 'n_bad': a[2], 'check_edge': a[3], 'build_ms': t[:, 0], 'check_ms': t[:, 1]}

    def itab_detail(self, slot):
        """1-D integral table of `slot`: {'log2_lo', 'ppo', 'd0', 'n_pan', 'by_fn' [15], 'by_pan'
        [n_pan], 'by_pan_edge' [n_pan], 'accepted_panels'} -- the worst deviation at the check points per function and per
        lambda panel (`by_pan_edge`: at the point near the panel edge alone) (panel p covers lambda in 2^(log2_lo + [p, p + 1] / ppo)) and the run of panels
        [lo, hi) that passed the gate (None: table rejected); None for a slot without such a table."""
        n = self.lib.cpol_debug_read(self.h, ('itab_detail%d' % slot).encode(), None, 0)
        if n == 0:
            return None
        nb = -int(n) - 1000
        if nb <= 0:
            self._check(int(n), 'cpol_debug_read(itab_detail)')
        v = self.debug_read('itab_detail%d' % slot, (nb // 8,), np.float64)
        n_pan = int(v[3])
        acc = v[19 + 2 * n_pan:19 + 2 * n_pan + 2]
        return {'log2_lo': v[0], 'ppo': int(v[1]), 'd0': v[2], 'n_pan': n_pan, 'by_fn': v[4:19],
                'by_pan': v[19:19 + n_pan], 'by_pan_edge': v[19 + n_pan:19 + 2 * n_pan],
                'accepted_panels': (int(acc[0]), int(acc[1])) if len(acc) == 2 else None}

    def debug_math(self, op, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        self._check(self.lib.cpol_debug_math(self.h, int(op), _ptr(x), _ptr(y), x.size),
                    'cpol_debug_math')
        return y

    def debug_scan(self, form, mul, x):
        """The kernels' own range scan of every row of x [n_rows, n] float32: form 1 the wavefront form, 0 the one-lane loop; mul:
        running product, else running sum."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError('debug_scan: x must be [n_rows, n]')
        y = np.empty_like(x)
        self._check(self.lib.cpol_debug_scan(self.h, int(form), int(bool(mul)), _ptr(x), _ptr(y), x.shape[0], x.shape[1]),
                    'cpol_debug_scan')
        return y

    def debug_shadow(self, mask, vals):
        """k_terrain_shadow alone (the test hook cpol_debug_read "terrain_shadow_rows"): mask [n_rows, n_gates] int8 codes and vals [n_vars, n_rows, n_gates] float32
        -> their shadowed copies (cosmo_pol_amd/shadow.py states the rule)."""
        mask = np.array(mask, dtype=np.int8, order='C')
        vals = np.array(vals, dtype=np.float32, order='C')
        if mask.ndim != 2 or vals.ndim != 3 or vals.shape[1:] != mask.shape:
            raise ValueError('debug_shadow: mask [n_rows, n_gates] and vals [n_vars, n_rows, n_gates]')
        class Hook(C.Structure):
            _fields_ = [('n_rows', C.c_int32), ('n_gates', C.c_int32), ('n_vars', C.c_int32), ('pad_', C.c_int32),
                        ('mask', C.c_void_p), ('vals', C.c_void_p)]
        h = Hook(mask.shape[0], mask.shape[1], vals.shape[0], 0, mask.ctypes.data, vals.ctypes.data)
        self._check(int(self.lib.cpol_debug_read(self.h, b'terrain_shadow_rows', C.byref(h), C.sizeof(h))),
                    'cpol_debug_read(terrain_shadow_rows)')
        return mask, vals

    def superob_fields(self, fields, spec, rays_per_block=0, want=None):
        """Test hook (cpol_debug_read "superob_fields"): k_superob on caller-supplied per-gate arrays {name: [n_rows, n_gates]}
        of SUPEROB_FIELDS (float32; RVEL float64; ZDR is made from ZH and ZV) -> what superob.average returns for them: the
        kernel on inputs no sweep produces.  `spec`: a superob.Superob.  `want`: the fields to ask the library for (default:
        those whose inputs are given)."""
        class Hook(C.Structure):
            _fields_ = [('n_rows', C.c_int32), ('n_gates', C.c_int32), ('inp', C.c_void_p * len(SUPEROB_FIELDS)), ('so', Superob)]
        h = Hook()
        keep, shape = [], None
        for i, k in enumerate(SUPEROB_FIELDS):
            if k == 'ZDR' or k not in fields:
                continue
            a = np.ascontiguousarray(fields[k], dtype=np.float64 if k == 'RVEL' else np.float32)
            if a.ndim != 2 or (shape is not None and a.shape != shape):
                raise ValueError('superob_fields: every field is [n_rows, n_gates]')
            shape = a.shape
            keep.append(a)
            h.inp[i] = a.ctypes.data
        if shape is None:
            raise ValueError('superob_fields: no field given')
        h.n_rows, h.n_gates = shape
        h.so.ray_window, h.so.gate_window, h.so.rays_per_block = spec.rays, spec.gates, int(rays_per_block)
        h.so.min_valid_fraction = spec.min_valid_fraction
        rpb = int(rays_per_block) or shape[0]
        if rpb < 1 or shape[0] % rpb:
            raise ValueError('superob_fields: rays_per_block %r does not divide %d rows' % (rays_per_block, shape[0]))
        wshape = ((shape[0] // rpb) * (-(-rpb // spec.rays)), -(-shape[1] // spec.gates))
        asked = [k for k in SUPEROB_FIELDS if (k in fields if k != 'ZDR' else ('ZH' in fields and 'ZV' in fields))]
        if want is not None:
            asked = [k for k in SUPEROB_FIELDS if k in want]
        out = {k: np.empty(wshape, dtype=np.float64 if k == 'RVEL' else np.float32) for k in asked}
        cnt = np.zeros((len(SUPEROB_FIELDS),) + wshape, dtype=np.uint16)
        for k, a in out.items():
            setattr(h.so, k, a.ctypes.data)
        h.so.count = cnt.ctypes.data
        rc = int(self.lib.cpol_debug_read(self.h, b'superob_fields', C.byref(h), C.sizeof(h)))
        self._check(rc, 'cpol_debug_read(superob_fields)')
        del keep
        out['count'] = {k: cnt[SUPEROB_FIELDS.index(k)] for k in asked}
        return out

    @staticmethod
    def histogram_struct(spec, phase=3, rays_per_block=0, model_index=None):
        """(Histogram for a call under `spec` (a histogram.Histogram), the arrays it points into): the edges as the caller gave
        them (float64; the library rounds them), the counts pointers the caller's.  model_index: the row of model_vars an
        ordinate ('model', name) stands for."""
        from . import histogram as HG
        h = Histogram()
        h.fields, h.phase, h.rays_per_block = spec.mask, int(phase), int(rays_per_block)
        keep = []
        for k in spec.fields:
            e = np.ascontiguousarray(spec.given[k], dtype=np.float64)
            keep.append(e)
            h.n_x[HISTOGRAM_FIELDS.index(k)] = len(e) - 1
            h.edges_x[HISTOGRAM_FIELDS.index(k)] = e.ctypes.data
        o = spec.ordinate
        if o is not None:
            if isinstance(o, tuple):
                if model_index is None or int(model_index) < 0:
                    raise ValueError('histogram: the ordinate %r needs the index of its model variable' % (o,))
                h.ordinate = HG.ORD_MODEL + int(model_index)
            else:
                h.ordinate = {'heights': HG.ORD_HEIGHTS, 'dist': HG.ORD_DIST}.get(o, HG.ORD_FIELD + HISTOGRAM_FIELDS.index(o) if o in HISTOGRAM_FIELDS else -1)
            e = np.ascontiguousarray(spec.ordinate_given, dtype=np.float64)
            keep.append(e)
            h.n_y, h.edges_y = len(e) - 1, e.ctypes.data
        return h, keep

    def histogram_stretch(self):
        """The gates a workgroup of k_hist owns (cpol_debug_read "histogram_stretch")."""
        v = C.c_int32(0)
        n = int(self.lib.cpol_debug_read(self.h, b'histogram_stretch', C.byref(v), 4))
        if n != 4:
            self._check(n, 'cpol_debug_read(histogram_stretch)')
        return int(v.value)

    def histogram_fields(self, per_gate, spec, rays_per_block=0, phase=3, tamper=None):
        """Test hook (cpol_debug_read "histogram_fields"): k_hist and the context's running state on caller-supplied rows ->
        what histogram.count returns for them.  per_gate: {field: [..., n_gates]} (float32; RVEL float64; leading axes are
        rows), 'heights' / 'dist' [n_rays, n_gates] (n_rays divides the rows), 'model_vars' {name: like a field, float64} --
        whatever is given is handed over; `spec`: a histogram.Histogram.  `tamper(h)`: changes the cpol_histogram before the
        call (the refusal tests).  A finishing call returns {field: uint64 counts}, any other None."""
        from . import histogram as HG

        class Hook(C.Structure):
            _fields_ = [('n_rows', C.c_int32), ('n_gates', C.c_int32), ('n_rays', C.c_int32), ('n_model_vars', C.c_int32),
                        ('inp', C.c_void_p * len(HISTOGRAM_FIELDS)), ('heights', C.c_void_p), ('dist', C.c_void_p),
                        ('model_vars', C.c_void_p), ('h', Histogram)]
        hk = Hook()
        keep, shape = [], None
        for i, k in enumerate(HISTOGRAM_FIELDS):
            if k not in per_gate:
                continue
            a = np.ascontiguousarray(per_gate[k], dtype=HG.dtype_of(k))
            a = a.reshape(-1, a.shape[-1])
            if shape is not None and a.shape != shape:
                raise ValueError('histogram_fields: every field has the same rows and gates')
            shape = a.shape
            keep.append(a)
            hk.inp[i] = a.ctypes.data
        if shape is None:
            raise ValueError('histogram_fields: no field given')
        hk.n_rows, hk.n_gates = shape
        hk.n_rays = shape[0]
        for k in ('heights', 'dist'):
            if k in per_gate:
                a = np.ascontiguousarray(per_gate[k], dtype=np.float32)
                a = a.reshape(-1, a.shape[-1])
                if a.shape[1] != shape[1] or (hk.n_rays != shape[0] and hk.n_rays != a.shape[0]):
                    raise ValueError('histogram_fields: heights and dist are [n_rays, n_gates]')
                hk.n_rays = a.shape[0]
                keep.append(a)
                setattr(hk, k, a.ctypes.data)
        names = list(per_gate.get('model_vars', {}))
        if names:
            mv = np.ascontiguousarray(np.stack([np.asarray(per_gate['model_vars'][n], dtype=np.float64).reshape(shape) for n in names]))
            keep.append(mv)
            hk.n_model_vars, hk.model_vars = len(names), mv.ctypes.data
        mi = names.index(spec.ordinate[1]) if isinstance(spec.ordinate, tuple) and spec.ordinate[1] in names else None
        hk.h, ekeep = self.histogram_struct(spec, phase, rays_per_block, model_index=mi if mi is not None else 0)
        keep += ekeep
        nb = 1 if not int(rays_per_block) or int(rays_per_block) < 0 or shape[0] % int(rays_per_block) else shape[0] // int(rays_per_block)
        out = {}
        if int(phase) & 2:
            for k in spec.fields:
                sh = (nb, len(spec.edges[k]) + 1) if spec.ordinate is None else (nb, spec.n_y_cells, len(spec.edges[k]) + 1)
                out[k] = np.full(sh, 0xDEADBEEF, dtype=np.uint64)
                hk.h.counts[HISTOGRAM_FIELDS.index(k)] = out[k].ctypes.data
        if tamper is not None:
            keep.append(tamper(hk.h))
        rc = int(self.lib.cpol_debug_read(self.h, b'histogram_fields', C.byref(hk), C.sizeof(hk)))
        self._check(rc, 'cpol_debug_read(histogram_fields)')
        del keep
        return out if int(phase) & 2 else None

    @staticmethod
    def composite_struct(spec, phase=3, rays_per_block=0, azimuths=None, gate_xy=None, source=0, plane_version=0):
        """(Composite for a call under `spec` (a composite.Composite), the arrays it points into): the edges, the thresholds and
        the slab as the caller gave them (float64; the library rounds thresholds and slab), ray_sin / ray_cos of `azimuths`
        (degrees; None leaves them NULL), the output pointers the caller's.  gate_xy = (x, y), float64 arrays of the call's
        geometry: the gate plane (CPOL_COMP_PLANE_GATES), kept on the device under `plane_version` when that is non-zero;
        `source`: this call's number for the source_of_* planes.  A spec with 'sum': the struct is a CompositeSums (its member
        `c` is the Composite, which shares its memory) with the weight tables set."""
        from . import composite as CP
        wide = CompositeSums() if CP.SUM in spec.products else None
        c = wide.c if wide is not None else Composite()
        c.fields, c.phase, c.products, c.rays_per_block = spec.mask, int(phase), spec.product_mask, int(rays_per_block)
        c.n_x, c.n_y = spec.n_x, spec.n_y
        keep = [spec.x_edges, spec.y_edges]
        c.edges_x, c.edges_y = spec.x_edges.ctypes.data, spec.y_edges.ctypes.data
        if spec.height_range is not None:
            c.use_slab, c.h_lo, c.h_hi = 1, spec.height_range_given[0], spec.height_range_given[1]
        for k in spec.fields:
            i = COMPOSITE_FIELDS.index(k)
            t = spec.thresholds_given[k]
            c.n_thresholds[i] = len(t)
            for j, v in enumerate(t):
                c.thresholds[i][j] = float(v)
        if azimuths is not None:
            rs, rc = CP.ray_tables(azimuths)
            rs, rc = np.ascontiguousarray(rs), np.ascontiguousarray(rc)
            keep += [rs, rc]
            c.ray_sin, c.ray_cos = rs.ctypes.data, rc.ctypes.data
        if gate_xy is not None:
            gx, gy = (np.ascontiguousarray(a, dtype=np.float64) for a in gate_xy)
            if gx.shape != gy.shape:
                raise ValueError('gate_xy: x %r and y %r differ in shape' % (gx.shape, gy.shape))
            keep += [gx, gy]
            c.plane, c.gate_x, c.gate_y, c.plane_version = 1, gx.ctypes.data, gy.ctypes.data, int(plane_version)
        c.source = int(source)
        if spec.n_z:
            c.n_z, c.edges_z, c.gaps = spec.n_z, spec.z_edges_given.ctypes.data, CP.GAPS.index(spec.gaps)
            keep.append(spec.z_edges_given)
            for k, (tv, tf) in spec.column.items():
                i = COMPOSITE_FIELDS.index(k)
                c.n_table[i], c.table_v[i], c.table_f[i] = len(tv), tv.ctypes.data, tf.ctypes.data
                keep += [tv, tf]
        if wide is not None:
            for k, (tv, tf) in spec.weight.items():
                i = COMPOSITE_FIELDS.index(k)
                wide.n_weight[i], wide.weight_v[i], wide.weight_f[i] = len(tv), tv.ctypes.data, tf.ctypes.data
                keep += [tv, tf]
            return wide, keep
        return c, keep

    def composite_plane(self):
        """(uploads, hits) of this context's gate-plane store (cpol_debug_read "composite_plane")."""
        v = (C.c_int64 * 2)()
        n = int(self.lib.cpol_debug_read(self.h, b'composite_plane', C.byref(v), 16))
        if n != 16:
            self._check(n, 'cpol_debug_read(composite_plane)')
        return int(v[0]), int(v[1])

    def composite_stretch(self):
        """The gates a workgroup of k_comp owns (cpol_debug_read "composite_stretch")."""
        v = C.c_int32(0)
        n = int(self.lib.cpol_debug_read(self.h, b'composite_stretch', C.byref(v), 4))
        if n != 4:
            self._check(n, 'cpol_debug_read(composite_stretch)')
        return int(v.value)

    def composite_fields(self, fields, dist, heights, azimuths, spec, rays_per_block=0, phase=3, lane_form=0, tamper=None,
                         gate_xy=None, source=0, plane_version=0):
        """Test hook (cpol_debug_read "composite_fields"): the plan, the placement, k_comp, k_comp_finish and the context's
        running state on caller-supplied rows -> what composite.finish returns for them.  fields: {field: float32 [..., n_gates]}
        (leading axes are rows); dist, heights: float32 [n_rays, n_gates] (n_rays divides the rows); azimuths [n_rays] degrees;
        `spec`: a composite.Composite; lane_form: 0 the kept form of k_comp, 1 lanes combined inside the wavefront, 2 every lane
        on its own.  `tamper(c)`: changes the cpol_composite before the call (the refusal tests).  gate_xy = (x, y), float64
        [n_rays, n_gates]: the gate plane (`dist` and `azimuths` may then be None), under `plane_version` in the plane store;
        `source`: the call's number.  A finishing call returns {'values': {field: {plane: array}}, 'count': {field: array}},
        any other None.  A spec with height layers: the planes and counts carry the layer axis ([n_blocks, n_z, n_y, n_x]), and
        with the product 'column' the result gains 'column' and 'column_layers' ({field: [n_blocks, n_y, n_x]}).  A spec with
        'sum': the call runs k_comp_sum (lane_form: 0 the kept form, 1 the runs of a wavefront summed first, 2 every lane on
        its own) and a finishing call k_comp_sum_finish; the result gains 'sum' (float64) and 'sum_skipped' (uint32), shaped
        like count[field]; `tamper` is given the CompositeSums."""
        from . import composite as CP
        with_sum = CP.SUM in spec.products

        class Hook(C.Structure):
            _fields_ = [('n_rows', C.c_int32), ('n_gates', C.c_int32), ('n_rays', C.c_int32), ('lane_form', C.c_int32),
                        ('inp', C.c_void_p * len(COMPOSITE_FIELDS)), ('heights', C.c_void_p), ('dist', C.c_void_p),
                        ('c', CompositeSums if with_sum else Composite)]
        hk = Hook()
        keep, shape = [], None
        for i, k in enumerate(COMPOSITE_FIELDS):
            if k not in fields:
                continue
            a = np.ascontiguousarray(fields[k], dtype=np.float32)
            a = a.reshape(-1, a.shape[-1])
            if shape is not None and a.shape != shape:
                raise ValueError('composite_fields: every field has the same rows and gates')
            shape = a.shape
            keep.append(a)
            hk.inp[i] = a.ctypes.data
        if shape is None:
            raise ValueError('composite_fields: no field given')
        hk.n_rows, hk.n_gates = shape
        geo = []
        for a in (heights if dist is None else dist, heights):
            a = np.ascontiguousarray(a, dtype=np.float32)
            a = a.reshape(-1, a.shape[-1])
            if a.shape[1] != shape[1] or shape[0] % a.shape[0] or (geo and geo[0].shape != a.shape):
                raise ValueError('composite_fields: heights and dist are [n_rays, n_gates], n_rays dividing the rows')
            geo.append(a)
        keep += geo
        hk.n_rays, hk.dist, hk.heights, hk.lane_form = geo[0].shape[0], geo[0].ctypes.data, geo[1].ctypes.data, int(lane_form)
        if dist is None:
            hk.dist = None
        if gate_xy is not None and any(np.size(a) != geo[1].size for a in gate_xy):
            raise ValueError('composite_fields: gate_xy are [n_rays, n_gates] like heights')
        hk.c, ckeep = self.composite_struct(spec, phase, rays_per_block, azimuths=azimuths, gate_xy=gate_xy, source=source,
                                            plane_version=plane_version)
        keep += ckeep
        hc = hk.c.c if with_sum else hk.c         # (the cpol_composite itself)
        sums, skipped = {}, {}
        rpb = int(rays_per_block)
        nb = 1 if rpb <= 0 or shape[0] % rpb else shape[0] // rpb
        vals, cnt, col, lay = {}, None, {}, {}
        z = (spec.n_z,) if spec.n_z else ()
        if int(phase) & 2:
            for k in spec.fields:
                vals[k] = np.full((nb,) + z + (len(spec.planes(k)), spec.n_y, spec.n_x), -7.0, dtype=np.float32)
                hc.values[COMPOSITE_FIELDS.index(k)] = vals[k].ctypes.data
            cnt = np.full((nb,) + z + (len(spec.fields), spec.n_y, spec.n_x), 0xDEADBEEF, dtype=np.uint64)
            hc.count = cnt.ctypes.data
            for k in spec.column:
                col[k] = np.full((nb, spec.n_y, spec.n_x), -7.0, dtype=np.float64)
                lay[k] = np.full((nb, spec.n_y, spec.n_x), 0xAB, dtype=np.uint8)
                hc.column[COMPOSITE_FIELDS.index(k)] = col[k].ctypes.data
                hc.column_layers[COMPOSITE_FIELDS.index(k)] = lay[k].ctypes.data
            for k in (spec.fields if with_sum else ()):
                sums[k] = np.full((nb,) + z + (spec.n_y, spec.n_x), -7.0, dtype=np.float64)
                skipped[k] = np.full((nb,) + z + (spec.n_y, spec.n_x), 0xDEADBEEF, dtype=np.uint32)
                hk.c.sum[COMPOSITE_FIELDS.index(k)] = sums[k].ctypes.data
                hk.c.sum_skipped[COMPOSITE_FIELDS.index(k)] = skipped[k].ctypes.data
        if tamper is not None:
            keep.append(tamper(hk.c))
        rc = int(self.lib.cpol_debug_read(self.h, b'composite_fields', C.byref(hk), C.sizeof(hk)))
        self._check(rc, 'cpol_debug_read(composite_fields)')
        del keep
        if not int(phase) & 2:
            return None
        if not spec.n_z:
            out = {'values': {k: {p: vals[k][:, j] for j, p in enumerate(spec.planes(k))} for k in spec.fields},
                   'count': {k: cnt[:, i] for i, k in enumerate(spec.fields)}}
        else:
            out = {'values': {k: {p: vals[k][:, :, j] for j, p in enumerate(spec.planes(k))} for k in spec.fields},
                   'count': {k: cnt[:, :, i] for i, k in enumerate(spec.fields)}}
            if spec.column:
                out['column'], out['column_layers'] = col, lay
        if with_sum:
            out['sum'], out['sum_skipped'] = sums, skipped
        return out

    @staticmethod
    def fractions_struct(spec):
        """(Fractions for a call under `spec` (a neighbourhood.Fractions), the arrays it points into): the field and the plane as
        indices, the thresholds as the caller gave them (float64; the library rounds them), the radii; `observed`, `domain` and
        the output pointers are the caller's."""
        f = Fractions()
        f.field, f.plane = COMPOSITE_FIELDS.index(spec.field), int(spec.plane_index)
        f.n_thresholds, f.n_radii = len(spec.thresholds_given), len(spec.radii)
        for j, v in enumerate(spec.thresholds_given):
            f.thresholds[j] = float(v)
        for j, r in enumerate(spec.radii):
            f.radii[j] = int(r)
        return f, []

    @staticmethod
    def objects_struct(spec, fractions, shifts=None):
        """(Objects for a call under `spec` (an objects.Objects), hung on `fractions` (the call's Fractions); what must stay alive):
        the output pointers are the caller's.  With spec.match the Objects is the first member of an ObjectsMatch, which is the
        first of what must stay alive and takes n_pieces, pieces and covered.  With spec.track that is in turn the first member
        of an ObjectsTrack, the first of what must stay alive, which takes the five arrays of the track; `shifts`: the given
        shifts of the call, int32 [n_blocks - 1, n_thr, 2] contiguous (objects.shifts_of_call), with spec.shifts."""
        if getattr(spec, 'track', False):
            ot = ObjectsTrack()
            o = ot.m.o                                # (shares ot's memory)
            o.pad_ = OBJ_TRACK | (spec.max_pieces if getattr(spec, 'match', False) else 0)
            ot.max_shift = -1 if spec.max_shift is None else spec.max_shift
            ot.max_pieces = spec.max_track_pieces
            keep = [ot]
            if spec.max_shift is None:
                ot.shifts_in = shifts.ctypes.data
                keep.append(shifts)
            fractions.objects = C.cast(C.pointer(ot), C.POINTER(Objects))
        elif getattr(spec, 'match', False):
            om = ObjectsMatch()
            o = om.o                                  # (shares om's memory)
            o.pad_ = spec.max_pieces
            fractions.objects = C.cast(C.pointer(om), C.POINTER(Objects))
            keep = [om]
        else:
            o = Objects()
            fractions.objects = C.pointer(o)
            keep = [o]
        o.connectivity, o.min_area, o.max_objects = spec.connectivity, spec.min_area, spec.max_objects
        if getattr(spec, 'sums', False):
            o.sums = 1
            if spec.weight is not None:
                tv, tf = (np.ascontiguousarray(spec.weight[0], dtype=np.float32), np.ascontiguousarray(spec.weight[1], dtype=np.float64))
                o.n_weight, o.weight_v, o.weight_f = len(tv), tv.ctypes.data, tf.ctypes.data
                keep += [tv, tf]
        return o, keep

    @staticmethod
    def probabilities_struct(fractions):
        """(the Fractions to hand to the library in place of `fractions`, the FractionProbabilities behind it; what must stay alive):
        `fractions` copied into a FractionsEnsemble, its n_radii flagged; the first result shares the wrapper's memory (pointers
        bound to it later are seen by the library), the output pointers are the caller's."""
        fe, q = FractionsEnsemble(), FractionProbabilities()
        fe.f = fractions
        fe.f.n_radii = fractions.n_radii | FRAC_ENSEMBLE
        fe.probabilities = C.pointer(q)
        return fe.f, q, [fe, q]

    def fractions_maps(self, maps, observed, spec, domain=None, tamper=None, objects=None, probabilities=None):
        """Test hook (cpol_debug_read "fractions_maps"): the checks and k_frac_rows, k_frac_cols, k_frac_score on caller-supplied
        maps -> what neighbourhood.sums returns for them.  maps: float32 [n_blocks, n_y, n_x] (or [n_y, n_x]); observed: float32
        [n_y, n_x]; domain: uint8 [n_y, n_x] or None; `spec`: a neighbourhood.Fractions, or any object with `thresholds_given`
        and `radii` (the maps need not be those of spec.composite's grid).  `tamper(f)`: changes the cpol_fractions before the call
        (the refusal tests).  `objects`: an objects.Objects or any object with `connectivity`, `min_area`, `max_objects` and
        `labels` (and `sums` with `weight` for the exact sums, `match` with `max_pieces` for the match, `track` with `max_shift`,
        `shifts` and `max_track_pieces` for the track, whose outputs are prefilled with 77): the kernels of
        cpol_obj.inl run too, and the result is (the sums, what objects.cells returns for the maps);
        `tamper` then finds the cpol_objects at f.objects.contents.  `probabilities`: a neighbourhood.Probabilities or any object
        with `maps` and `any_maps` (which of the two maps are wanted): k_frac_members runs too, and the result gains, as its last
        element, what neighbourhood.ensemble_sums returns for the maps; the cpol_fractions is then the first member of a
        cpol_fractions_ensemble, and `tamper` finds the cpol_fraction_probabilities as the Python attribute f.probabilities."""
        from . import neighbourhood as NB

        class Hook(C.Structure):
            # (f and the pointer behind it: a cpol_fractions_ensemble where f.n_radii says so)
            _fields_ = [('n_blocks', C.c_int32), ('n_y', C.c_int32), ('n_x', C.c_int32), ('pad_', C.c_int32), ('maps', C.c_void_p),
                        ('f', Fractions), ('probabilities', C.POINTER(FractionProbabilities))]
        m = np.ascontiguousarray(maps, dtype=np.float32)
        if m.ndim == 2:
            m = m[None]
        o = np.ascontiguousarray(observed, dtype=np.float32)
        if m.ndim != 3 or o.shape != m.shape[1:]:
            raise ValueError('fractions_maps: maps [n_blocks, n_y, n_x], observed [n_y, n_x]')
        keep = [m, o]
        hk = Hook()
        hk.n_blocks, hk.n_y, hk.n_x = m.shape
        hk.maps = m.ctypes.data
        f = Fractions()
        f.n_thresholds, f.n_radii = len(spec.thresholds_given), len(spec.radii)
        for j, v in enumerate(spec.thresholds_given):
            f.thresholds[j] = float(v)
        for j, r in enumerate(spec.radii):
            f.radii[j] = int(r)
        f.observed = o.ctypes.data
        if domain is not None:
            d = np.ascontiguousarray(domain, dtype=np.uint8)
            if d.shape != o.shape:
                raise ValueError('fractions_maps: domain [n_y, n_x]')
            keep.append(d)
            f.domain = d.ctypes.data
        nt, nr = f.n_thresholds, f.n_radii
        s = np.full((m.shape[0], nt, nr, 3), 0xDEADBEEF, dtype=np.uint64)
        t = np.full((m.shape[0], nt, 3), 0xDEADBEEF, dtype=np.uint64)
        f.sums, f.totals = s.ctypes.data, t.ctypes.data
        if objects is not None:
            from . import objects as OB
            with_track = getattr(objects, 'track', False)
            n_pairs = max(m.shape[0] - 1, 0)
            given = None
            if with_track and objects.max_shift is None:      # (a call of one block still reaches the library, which refuses it)
                given = np.ascontiguousarray(np.broadcast_to(objects.shifts, (max(n_pairs, 1), nt, 2)), dtype=np.int32)
            o, okeep = Context.objects_struct(objects, f, given)
            n_obj = np.full((m.shape[0] + 1, nt), 0xDEADBEEF, dtype=np.uint32)
            table = np.full((m.shape[0] + 1, nt, objects.max_objects, OBJ_WORDS), 0xDEADBEEF, dtype=np.uint32)
            o.n_objects, o.table = n_obj.ctypes.data, table.ctypes.data
            labels = None
            if objects.labels:
                labels = np.full((m.shape[0] + 1, nt) + m.shape[1:], -559038737, dtype=np.int32)
                o.labels = labels.ctypes.data
            osums = None
            if getattr(objects, 'sums', False):
                osums = [np.full((m.shape[0] + 1, nt, objects.max_objects, 3), np.nan, dtype=np.float64),
                         np.full((m.shape[0] + 1, nt, objects.max_objects), 0xDEADBEEF, dtype=np.uint32),
                         np.full((m.shape[0] + 1, 3), np.nan, dtype=np.float64), np.full((m.shape[0] + 1, 2), 0xDEADBEEF, dtype=np.uint32)]
                o.volume, o.skipped, o.field, o.field_cells = [q.ctypes.data for q in osums]
            omatch = None
            if getattr(objects, 'match', False):
                omatch = [np.full((m.shape[0], nt), 0xDEADBEEF, dtype=np.uint32),
                          np.full((m.shape[0], nt, objects.max_pieces, OBJ_WORDS), 0xDEADBEEF, dtype=np.uint32),
                          np.full((m.shape[0], nt, 2, objects.max_objects), 0xDEADBEEF, dtype=np.uint32)]
                om = okeep[0].m if with_track else okeep[0]
                om.n_pieces, om.pieces, om.covered = [q.ctypes.data for q in omatch]
            otrack = None
            if with_track:
                # (prefilled with 77: the zero rows are the library's, and a correlation that is not computed stays as it is)
                side = 2 * (objects.max_shift or 0) + 1
                otrack = [np.full((n_pairs, nt, side, side), 77, dtype=np.uint32), np.full((n_pairs, nt, 2), 77, dtype=np.int32),
                          np.full((n_pairs, nt), 77, dtype=np.uint32),
                          np.full((n_pairs, nt, objects.max_track_pieces, OBJ_WORDS), 77, dtype=np.uint32),
                          np.full((n_pairs, nt, 2, objects.max_objects), 77, dtype=np.uint32)]
                ot = okeep[0]
                ot.correlation, ot.shift, ot.n_pieces, ot.pieces, ot.covered = [q.ctypes.data for q in otrack]
            keep += okeep
        q = None
        if probabilities is not None:
            q = FractionProbabilities()
            f.n_radii |= FRAC_ENSEMBLE
            hk.probabilities = C.pointer(q)
            nb = m.shape[0]
            # (a refused call may carry more blocks than the table has rows for: the arrays stay those of the limit)
            pout = [np.full((nt, nr, 3), 0xDEADBEEF, dtype=np.uint64),
                    np.full((nt, nr, min(nb, FRAC_PROB_MAX_BLOCKS) + 1, 2), 0xDEADBEEF, dtype=np.uint64),
                    np.full((nt, nr) + m.shape[1:], 0xDEADBEEF, dtype=np.uint32) if probabilities.maps else None,
                    np.full((nt, nr) + m.shape[1:], 0xDEADBEEF, dtype=np.uint32) if probabilities.any_maps else None]
            q.prob_sums, q.reliability = pout[0].ctypes.data, pout[1].ctypes.data
            q.member_sum = pout[2].ctypes.data if pout[2] is not None else None
            q.member_any = pout[3].ctypes.data if pout[3] is not None else None
            keep += [q] + pout
        hk.f = f
        if tamper is not None:
            fv = hk.f                                 # (shares hk's memory)
            if q is not None:
                fv.probabilities = q                  # (a Python attribute: the struct itself has no such member)
            keep.append(tamper(fv))
        rc = int(self.lib.cpol_debug_read(self.h, b'fractions_maps', C.byref(hk), C.sizeof(hk)))
        self._check(rc, 'cpol_debug_read(fractions_maps)')
        del keep
        out = [NB.result(spec, s, t)]
        if objects is not None:
            # (given shifts: no correlation is delivered; the array the library was handed all the same is 'track_correlation_buffer')
            computed = otrack is not None and objects.max_shift is not None
            out.append(OB.result(_ObjectsNamed(objects, spec, m.shape[1:]), n_obj, table, labels, osums, omatch,
                                 otrack if otrack is None or computed else [None] + otrack[1:]))
            if otrack is not None and not computed:
                out[-1]['track_correlation_buffer'] = otrack[0]
        if probabilities is not None:
            out.append(NB.ensemble_result(spec, m.shape[0], *pout))
        return out[0] if len(out) == 1 else tuple(out)

    @staticmethod
    def spectrum_moments_struct(spec):
        """SpectrumMoments for a call under `spec` (a spectrum_moments.SpectrumMoments); the output pointers are the caller's."""
        sm = SpectrumMoments()
        sm.fields, sm.min_bins, sm.min_power = spec.mask, spec.min_bins, spec.min_power
        return sm

    def spectrum_moments_rows(self, spectrum, varray, spec, out=None):
        """Test hook (cpol_debug_read "spectrum_moments_rows"): k_spec_moments on caller-supplied spectra [n_rows, n_v]
        (float64, every row a gate) and velocity bins [n_v] -> what spectrum_moments.moments returns for them: the kernel on
        rows no sweep produces.  `spec`: a spectrum_moments.SpectrumMoments.  `out`: a float64 [8, n_rows] array the library
        writes the requested rows of (default: a fresh one); the result's arrays are its rows."""
        class Hook(C.Structure):
            _fields_ = [('n_rows', C.c_int32), ('n_v', C.c_int32), ('spectrum', C.c_void_p), ('varray', C.c_void_p),
                        ('sm', SpectrumMoments)]
        S = np.ascontiguousarray(spectrum, dtype=np.float64)
        V = np.ascontiguousarray(varray, dtype=np.float64)
        if S.ndim != 2 or V.ndim != 1 or S.shape[1] != V.shape[0]:
            raise ValueError('spectrum_moments_rows: spectrum is [n_rows, n_v], varray [n_v]')
        n_rows = S.shape[0]
        if out is None:
            out = np.empty((len(SPECTRUM_MOMENTS_FIELDS), n_rows), dtype=np.float64)
        if out.shape != (len(SPECTRUM_MOMENTS_FIELDS), n_rows) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError('spectrum_moments_rows: out is a contiguous float64 [8, n_rows] array')
        cnt = np.zeros(n_rows, dtype=np.uint16)
        h = Hook()
        h.n_rows, h.n_v = S.shape
        h.spectrum, h.varray = S.ctypes.data, V.ctypes.data
        h.sm = self.spectrum_moments_struct(spec)
        h.sm.moments, h.sm.count = out.ctypes.data, cnt.ctypes.data
        rc = int(self.lib.cpol_debug_read(self.h, b'spectrum_moments_rows', C.byref(h), C.sizeof(h)))
        self._check(rc, 'cpol_debug_read(spectrum_moments_rows)')
        res = {k: out[SPECTRUM_MOMENTS_FIELDS.index(k)] for k in spec.fields}
        res['count'] = cnt
        return res

    @staticmethod
    def species_struct(n_hydro):
        """Species for a call with `n_hydro` staged hydrometeor slots; the output pointers are the caller's."""
        sp = Species()
        sp.n_hydro = int(n_hydro)
        return sp

    def species_fields(self, sz, zh_final, c_zh, c_kdp, c_2w, want=None):
        """Test hook (cpol_debug_read "species_fields"): k_species alone on caller-supplied rows sz [n_rows, n_gates, n_hydro, 12]
        (float32) and zh_final [n_rows, n_gates] (float32) with the three float32 constants -> what species.fields_of returns
        for them: the kernel on rows no sweep produces.  `want`: the arrays to ask for, out of SPECIES_FIELDS, 'dominant',
        'present', 'share' and 'sz' (default: all); the others stay NULL in the struct.  The result holds the requested arrays,
        each allocated with a sentinel fill so that an array the library must not touch can be told from one it wrote."""
        class Hook(C.Structure):
            _fields_ = [('n_rows', C.c_int32), ('n_gates', C.c_int32), ('sz', C.c_void_p), ('zh_final', C.c_void_p),
                        ('c_zh', C.c_float), ('c_kdp', C.c_float), ('c_2w', C.c_float), ('pad_', C.c_float), ('sp', Species)]
        S = np.ascontiguousarray(sz, dtype=np.float32)
        Z = np.ascontiguousarray(zh_final, dtype=np.float32)
        if S.ndim != 4 or S.shape[3] != 12 or Z.shape != S.shape[:2]:
            raise ValueError('species_fields: sz is [n_rows, n_gates, n_hydro, 12], zh_final [n_rows, n_gates]')
        n_rows, n_gates, n_hydro = S.shape[:3]
        every = SPECIES_FIELDS + ['dominant', 'present', 'share', 'sz']
        want = every if want is None else list(want)
        for k in want:
            if k not in every:
                raise ValueError('species_fields: no array %r' % (k,))
        res = {}
        h = Hook()
        h.n_rows, h.n_gates = n_rows, n_gates
        h.sz, h.zh_final = S.ctypes.data, Z.ctypes.data
        h.c_zh, h.c_kdp, h.c_2w = float(c_zh), float(c_kdp), float(c_2w)
        h.sp = self.species_struct(n_hydro)
        for k in want:
            if k in SPECIES_FIELDS:
                res[k] = np.full((n_hydro, n_rows, n_gates), 12345.0, dtype=np.float32)
            elif k == 'share':
                res[k] = np.full((n_rows, n_gates), 12345.0, dtype=np.float32)
            elif k == 'sz':
                res[k] = np.full(S.shape, 12345.0, dtype=np.float32)
            else:
                res[k] = np.full((n_rows, n_gates), 0xA5, dtype=np.uint8)
            setattr(h.sp, k, res[k].ctypes.data)
        rc = int(self.lib.cpol_debug_read(self.h, b'species_fields', C.byref(h), C.sizeof(h)))
        self._check(rc, 'cpol_debug_read(species_fields)')
        return res

    @staticmethod
    def member_stats_struct(spec, names, phase, capacity=None):
        """(MemberStats for a call of a pass that folds the fields `names` under `spec` (an ensemble_stats.EnsembleStats),
        what keeps its threshold and quantile arrays alive).  `capacity`: the members the whole pass holds, read when `spec`
        is an EnsembleQuantiles (the device keeps that many rows per field with quantiles); None: the limit of 128."""
        ms = MemberStats()
        ms.phase, ms.min_members = int(phase), spec.min_members
        keep = []
        for k in names:
            i = MEMBER_STATS_FIELDS.index(k)
            ms.fields |= 1 << i
            thr = np.ascontiguousarray(spec.exceed.get(k, ()), dtype=np.float64)
            if thr.size:
                keep.append(thr)
                ms.n_thresholds[i], ms.thresholds[i] = thr.size, thr.ctypes.data
        qs = getattr(spec, 'quantiles', None)
        if qs or getattr(spec, 'verify', None):             # (a verified field keeps its members like a field with quantiles)
            from . import ensemble_stats as ES
            ms.quantile_capacity = ES.MAX_QUANTILE_MEMBERS if capacity is None else int(capacity)
            ms.quantile_method = ES.METHODS.index(spec.method)
        if qs:
            for k in names:
                if k in qs:
                    i = MEMBER_STATS_FIELDS.index(k)
                    q = np.ascontiguousarray(qs[k], dtype=np.float64)
                    keep.append(q)
                    ms.n_quantiles[i], ms.quantiles[i] = q.size, q.ctypes.data
        return ms, keep

    def member_stats_fields(self, fields, spec, phase=3, n_cells=None, names=None, capacity=None, _hook=None):
        """Test hook (cpol_debug_read "member_stats_fields"): the product's k_member_fold / k_member_finish and this context's
        running state on caller-supplied members {name: [n_members, n_cells]} of MEMBER_STATS_FIELDS (float32; RVEL float64).
        `spec`: an ensemble_stats.EnsembleStats; `phase`: bit 0 begins a pass, bit 1 finishes it -- a pass may be cut into
        calls; `fields` may be empty (no member; then `n_cells` and `names` say what the pass holds).  `capacity` (an
        EnsembleQuantiles): the members of the whole pass; None: those of this call, and at least 1.  A finishing call
        returns what ensemble_stats.finish returns ('quantile' included when `spec` asks for quantiles), every other call
        None."""
        class Hook(C.Structure):
            _fields_ = [('n_members', C.c_int32), ('n_cells', C.c_int64), ('inp', C.c_void_p * len(MEMBER_STATS_FIELDS)),
                        ('ms', MemberStats)]
        # (_hook: member_verify_fields' struct, which begins like this one, and its control name)
        h, control = _hook if _hook is not None else (Hook(), b'member_stats_fields')
        keep, shape = [], None
        for i, k in enumerate(MEMBER_STATS_FIELDS):
            if k not in fields:
                continue
            a = np.ascontiguousarray(fields[k], dtype=np.float64 if k == 'RVEL' else np.float32)
            if a.ndim != 2 or (shape is not None and a.shape != shape):
                raise ValueError('member_stats_fields: every field is [n_members, n_cells]')
            shape = a.shape
            keep.append(a)
            h.inp[i] = a.ctypes.data
        if names is None:
            names = spec.resolve([k for k in MEMBER_STATS_FIELDS if k in fields])
        if shape is None:
            shape = (0, int(n_cells))
        h.n_members, h.n_cells = shape
        h.ms, thr_keep = self.member_stats_struct(spec, names, phase, capacity=max(shape[0], 1) if capacity is None else capacity)
        out = None
        if int(phase) & 2:
            nc = shape[1]
            out = {kind: {k: np.empty(nc, dtype=np.float64 if k == 'RVEL' else np.float32) for k in names} for kind in spec.kinds}
            cnt = np.zeros((len(MEMBER_STATS_FIELDS), nc), dtype=np.uint16)
            out['exceed'] = {k: np.empty((len(spec.exceed[k]), nc), dtype=np.uint16) for k in names if k in spec.exceed}
            for k in names:
                i = MEMBER_STATS_FIELDS.index(k)
                for kind in spec.kinds:
                    getattr(h.ms, kind)[i] = out[kind][k].ctypes.data
                if k in out['exceed']:
                    h.ms.exceed[i] = out['exceed'][k].ctypes.data
            h.ms.count = cnt.ctypes.data
            qs = getattr(spec, 'quantiles', None)
            if qs:
                out['quantile'] = {k: np.empty((len(qs[k]), nc), dtype=np.float64 if k == 'RVEL' else np.float32) for k in names if k in qs}
                for k, a in out['quantile'].items():
                    h.ms.quantile[MEMBER_STATS_FIELDS.index(k)] = a.ctypes.data
        rc = int(self.lib.cpol_debug_read(self.h, control, C.byref(h), C.sizeof(h)))
        self._check(rc, 'cpol_debug_read(%s)' % control.decode())
        del keep, thr_keep
        if out is not None:
            out['count'] = {k: cnt[MEMBER_STATS_FIELDS.index(k)] for k in names}
        return out

    @staticmethod
    def member_verify_struct(spec):
        """MemberVerify for a call of a pass under `spec` (an ensemble_verify.EnsembleVerification): fields and fair, which go
        with every call; the observation and output pointers are the finishing call's."""
        mv = MemberVerify()
        for k in spec.verify:
            mv.fields |= 1 << MEMBER_STATS_FIELDS.index(k)
        mv.fair = int(spec.fair)
        return mv

    def member_verify_fields(self, fields, observations, spec, phase=3, n_cells=None, names=None, capacity=None):
        """Test hook (cpol_debug_read "member_verify_fields"): member_stats_fields with a verification beside it
        (k_member_verify).  `spec`: an ensemble_verify.EnsembleVerification; `observations` {name: [n_cells]} of the verified
        fields (read by a finishing call; None otherwise).  A finishing call returns what ensemble_verify.finish returns, every
        other call None."""
        class Hook(C.Structure):
            _fields_ = [('n_members', C.c_int32), ('n_cells', C.c_int64), ('inp', C.c_void_p * len(MEMBER_STATS_FIELDS)),
                        ('ms', MemberStats), ('mv', MemberVerify)]
        h = Hook()
        h.mv = self.member_verify_struct(spec)
        keep = []
        if int(phase) & 2:
            nc = int(n_cells) if not fields else np.shape(next(iter(fields.values())))[1]
            ver = {'below': {}, 'equal': {}, 'crps': {}}
            for k in spec.verify:
                i = MEMBER_STATS_FIELDS.index(k)
                T = np.float64 if k == 'RVEL' else np.float32
                y = np.ascontiguousarray(observations[k], dtype=T)
                if y.shape != (nc,):
                    raise ValueError('member_verify_fields: every observation is [n_cells]')
                keep.append(y)
                h.mv.obs[i] = y.ctypes.data
                for kind, dt in (('below', np.uint16), ('equal', np.uint16), ('crps', T)):
                    ver[kind][k] = np.empty(nc, dtype=dt)
                    getattr(h.mv, kind)[i] = ver[kind][k].ctypes.data
        out = self.member_stats_fields(fields, spec, phase=phase, n_cells=n_cells, names=names, capacity=capacity,
                                       _hook=(h, b'member_verify_fields'))
        del keep
        if out is not None:
            out['verify'] = ver
        return out

    FORM_NAMES = ('g1r', 'gate1_ray', 'gate1', 'interp_classify', 'rare_direct', 'subbeam_sum', 'final_inplace',
                  'poly_central', 'n_sub', 'lanes_alive', 'scan_form', 'graph_replayed')

    def launch_forms(self):
        """Which launch sequence the last cpol_run_sweep of this context took (tests / bench result checks): {name: int}."""
        v = self.debug_read('launch_forms', (len(self.FORM_NAMES),), np.int32)
        return dict(zip(self.FORM_NAMES, (int(x) for x in v)))

    # enum WorkBuf of csrc/cpol_buffers.h, in its order
    WORK_BUFFERS = ('traj', 'rayc', 'poly', 'timed', 'vals', 'mask', 'elev', 'coords', 'wgate', 'qmelt', 'fwmelt',
                    'key', 'pos', 'par', 'count', 'totals', 'blkranked', 'rec', 'vmask', 'offset', 'perm', 'res',
                    'vn', 'icefirst', 'proj', 'colin', 'xscr', 'xgeo', 'beam', 'bsigma', 'bon',
                    'gscan', 'defer', 'present', 'ticket', 'units', 'szinteg', 'clk')

    def work_buffers(self):
        """The capacity in bytes of every per-sweep work buffer of this context, 0 where it is absent (a test hook): {name: int}."""
        v = self.debug_read('work_buffers', (len(self.WORK_BUFFERS),), np.uint64)
        return dict(zip(self.WORK_BUFFERS, (int(x) for x in v)))

    def debug_read(self, name, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        n = self.lib.cpol_debug_read(self.h, name.encode(), _ptr(out), out.nbytes)
        if n < 0:
            self._check(int(n), 'cpol_debug_read(%s)' % name)
        if n != out.nbytes:
            raise NativeError('cpol_debug_read(%s): got %d bytes, expected %d'
                              % (name, n, out.nbytes))
        return out
