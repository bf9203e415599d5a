/* cosmo_pol_amd.h -- C ABI of the MI355X-native cosmo_pol hot path.
 *
 * Shared library: cosmo_pol_amd/csrc/libcosmo_pol_hip.so (hipcc, gfx950).
 * Plain C: opaque context, raw pointers and sizes, int status codes
 * (0 = ok, < 0 = error; text via cpol_last_error).  Never throws / aborts.
 * The caller owns every host buffer; device copies are owned by the context.
 * A context is NOT thread-safe: one per GPU per process (one process per GPU,
 * sweeps sharded by rays).
 *
 * What each entry point replaces in the reference (wolfidan/cosmo_pol):
 *
 *   cpol_stage_model    pycosmo variables handed to the workers through module
 *                       globals (radar_operator.py:199-215) and re-read for
 *                       every radial and variable by the SWIG call
 *                       (interpolation/interpolation.py:584-595)
 *   cpol_stage_hydro    Lookup_table objects of load_all_lut (lookup/lut.py:
 *                       27-76) + create_hydrometeor constants
 *                       (hydrometeors/hydrometeors.py:39, doppler_scatter.py:
 *                       111-122)
 *   cpol_interp_points  the native gate kernel itself, same inputs as
 *                       get_all_radar_pts (interpolation/interpolation_c.c:8)
 *                       but evaluated for every staged variable in one pass
 *   cpol_run_sweep      the body of the scan loop: for every radial
 *                       get_interpolated_radial (interpolation/interpolation.py:
 *                       91) -> melting (interpolation/melting.py:19) ->
 *                       get_radar_observables (scatter/doppler_scatter.py:49)
 *                       -> integrate_radials (interpolation.py:36), and
 *                       cut_at_sensitivity (doppler_scatter.py:804) for the
 *                       whole sweep: ONE call per sweep instead of one
 *                       pool.map task per radial (radar_operator.py:429-432)
 *   cpol_stage_member, cpol_num_members, cpol_select_member, cpol_run_sweep_members
 *                       nothing: the reference runs one model state per process (one
 *                       RadarOperator, one load_model_file; an ensemble is a shell loop
 *                       that reloads the lookup tables for every member)
 */
#ifndef COSMO_POL_AMD_H
#define COSMO_POL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the cpol_* functions below are its only exported symbols. */
#if defined(__GNUC__)
#define CPOL_API __attribute__((visibility("default")))
#else
#define CPOL_API
#endif

typedef struct cpol_ctx cpol_ctx;

enum {
    CPOL_OK = 0,
    CPOL_ERR_HIP = -1,          /* a HIP runtime call failed            */
    CPOL_ERR_ARG = -2,          /* invalid argument / not staged        */
    CPOL_ERR_DOMAIN = -3,       /* a gate lies outside the model domain
                                   (reference: IndexError,
                                   interpolation.py:572-580)            */
    CPOL_ERR_NOMEM = -4
};

#define CPOL_MAX_VARS   24
#define CPOL_MAX_HYDRO  8
#define CPOL_N_SZ       12      /* columns of a LUT row (compute_lut_sz.py:265-297) */
#define CPOL_MAX_GATES  5460    /* gates of a ray: the operands of its three range scans (3 x n_gates float32) lie in the
                                   64 KB of LDS a workgroup may ask for, 16 bytes of which stay with the scan kernels'
                                   own variables; more gates: CPOL_ERR_ARG before anything is launched */
#define CPOL_TRAJ_STRIDE 4      /* doubles per (ray, vertical node) entry of the `traj` table */
#define CPOL_GEO_STRIDE  8      /* doubles per (ray, horizontal node) entry of the `geo` table */
#define CPOL_SITE_STRIDE 8      /* doubles per ray of the `site` table */

/* PSD families (how N(D) is evaluated on the device) */
enum {
    CPOL_PSD_GAMMA = 0,         /* N0 D^mu exp(-lambda D^nu)   hydrometeors.py:128-147 */
    CPOL_PSD_ICE_FIELD = 1,     /* 1-moment ice, Field (2005)  hydrometeors.py:1231-1373 */
    CPOL_PSD_MELTING = 2        /* melting snow / graupel      hydrometeors.py:303-478  */
};

/* how (lambda, N0) follow from the model moments */
enum {
    CPOL_RULE_RAIN_1MOM = 0,    /* hydrometeors.py:747-772   */
    CPOL_RULE_SNOW_1MOM = 1,    /* hydrometeors.py:879-907   */
    CPOL_RULE_GRAUPEL_1MOM = 2, /* hydrometeors.py:1025-1049 */
    CPOL_RULE_TWO_MOMENT = 3,   /* hydrometeors.py:212-256, 1341-1365 */
    CPOL_RULE_ICE_1MOM = 4,     /* hydrometeors.py:1302-1339 */
    CPOL_RULE_MELTING_SNOW = 5, /* hydrometeors.py:1398-1434 */
    CPOL_RULE_MELTING_GRAUPEL = 6 /* hydrometeors.py:1446-1481 */
};

/* mass source of a hydrometeor slot */
enum {
    CPOL_Q_MODEL = 0,           /* a staged model variable (var_q)             */
    CPOL_Q_MELT_SNOW = 1,       /* QmS_v diagnosed by the melting scheme       */
    CPOL_Q_MELT_GRAUPEL = 2     /* QmG_v                                       */
};

typedef struct {
    int32_t psd_family;         /* CPOL_PSD_*  */
    int32_t rule;               /* CPOL_RULE_* */
    int32_t q_source;           /* CPOL_Q_*    */
    int32_t var_q;              /* staged-variable index of the mass density   */
    int32_t var_qn;             /* ... of the number density (2-moment) or -1  */
    int32_t var_t;              /* ... of the temperature                      */
    int32_t n_e, n_t, n_d;      /* table shape [n_e, n_t, n_d, 12]             */
    int32_t second_axis_f64;    /* 1: second axis queried with a float64 value
                                   (wet fraction), 0: float32 (temperature)    */
    float   e_lo, e_step;       /* axes_limits[0][0], axes_step[0]  (float32)  */
    float   t_lo, t_step;       /* second axis ('t' or 'wc')        (float32)  */
    double  dD;                 /* d axis step D[1]-D[0] (as float32 value)    */
    /* generic power-law / PSD constants (python-float values of the reference) */
    double  a, b, alpha, beta, mu, nu;
    double  lambda_factor, ntot_factor, vel_factor;
    double  n0_fixed;           /* rain / graupel 1-mom intercept (0 if per gate) */
    double  x_min, x_max;       /* 2-moment mean-mass clip                     */
    double  c_n0, c_lam;        /* 2-moment unit factors 1000^-(1+mu), 1000^-nu */
    double  lam_exponent;       /* 1/(4+mu) | 1/(b+1) | -nu/b                  */
    double  n0_exponent;        /* (mu+1)/nu (2-moment)                        */
    /* melting species: rain and dry-solid partners                            */
    double  r_a, r_b, r_alpha, r_beta, r_n0, r_mu, r_lambda_factor, r_lam_exponent;
    double  r_dmin, r_dmax, s_dmin, s_dmax;
    int32_t solid_rule;         /* CPOL_RULE_SNOW_1MOM or _GRAUPEL_1MOM        */
    int32_t uniform_grid;       /* gamma family, nu == 1: aux[] holds the grid step
                                   and per-bin offsets for the exp recurrence   */
    int32_t numeric_intv;       /* gamma family whose fall-speed moments are summed
                                   numerically over ALL gates (2-moment ice,
                                   hydrometeors.py:1256-1275): aux[] = D^mu, D^nu,
                                   V(D) on the linspace grid, then its step       */
    int32_t tab_degree;         /* 0, or the degree of the polynomial tables appended to aux[]:
                                   melting family (CPOL_MELT_DEGREE): per wet-fraction bin of
                                   the table's second axis and diameter bin, polynomials in
                                   the wet fraction of the four fw-only factors of N(D);
                                   1-moment ice (CPOL_ICE_DEGREE): per panel in log2(lambda),
                                   polynomials of the three normalisation sums (which depend on
                                   lambda only).  See cpol_stage_hydro                     */
    int32_t pad_;
    uint64_t table_id;          /* 0, or a caller-chosen identity of EVERYTHING staged for this
                                   slot (descriptor, table, per-bin factors, aux, Doppler
                                   weights): the integral tables built for an id are kept (the
                                   CPOL_ITAB_CACHE most recent) and reused when a slot with the
                                   same id is staged again -- a caller that switches between a
                                   few table sets (Ku / Ka / ground radar, get_GPM_swath) pays
                                   for their construction once.  Equal ids must mean equal
                                   content                                                 */
} cpol_hydro_desc;
#define CPOL_ITAB_CACHE 24

#define CPOL_MELT_DEGREE 10     /* degree of those polynomials (11 coefficients)           */
#define CPOL_MELT_FUNCS  4      /* D_r, G, G*M, G*V                                        */
#define CPOL_ICE_DEGREE  10     /* degree of the ice normalisation-sum polynomials         */
#define CPOL_ICE_FUNCS   3      /* sum a D^b phi, sum V phi, sum phi over the norm. grid   */

typedef struct {
    int32_t n_rays, n_gates;
    int32_t n_sub;              /* kept antenna-quadrature points per radial    */
    int32_t n_hnodes, n_vnodes; /* distinct horizontal / vertical GH nodes      */
    int32_t with_melting, with_attenuation;
    int32_t integrate_model;    /* also return antenna-averaged model variables */
    int32_t apply_sensitivity;  /* 1: censor with tables->sens_thr (cut_at_sensitivity) */
    int32_t outputs_on_device;  /* 0: output pointers are host buffers, the call returns when
                                   they are filled; 1: device pointers, the kernels write
                                   them in place, the call returns at once; 2: PINNED host
                                   buffers (cpol_host_alloc), device-to-host copies are queued
                                   on the context's stream and the call returns at once --
                                   results (and a deferred CPOL_ERR_DOMAIN) after
                                   cpol_synchronize.  Carve the arrays from ONE allocation:
                                   when they span a window of at most 1.25 x their total
                                   size they are moved by a single copy (which also
                                   overwrites the padding bytes between them -- do not keep
                                   other data inside that window).  Every array must be
                                   aligned to its element size, as any C array is            */
    int32_t simulate_doppler;   /* 0 off, 1 / 2 / 3 = Doppler scheme of the reference (RVEL;
                                   3 = full Doppler spectrum, doppler_scatter.py:335-391) */
    int32_t geometry_mode;      /* CPOL_GEOM_*                                   */
    double  radar_lat, radar_lon, radar_alt;
    double  range0, range_step; /* RANGE_RADAR = range0 + k*range_step          */
    double  ke, re;             /* 4/3 and the earth radius (host evaluates quirk Q1) */
    double  sin_u1, cos_u1;     /* reduced latitude of the radar (Vincenty)     */
    double  wavelength;         /* mm                                           */
    double  k_squared;
    double  radial_res;         /* m                                            */
    double  c_zh;               /* wavelength^4 / (pi^5 K^2)                     */
    int32_t var_u, var_v, var_w; /* staged-variable indices of the wind (RVEL)    */
    int32_t var_rho;            /* ... of the air density (Doppler scheme 3) or -1 */
    /* Doppler scheme 3 */
    int32_t n_vbins;            /* len(VARRAY) = FFT_length + 1 (global_constants.py:171) */
    int32_t debug_flags;        /* 0 in production.  CPOL_DEBUG_EXACT_SUBBEAMS (bit 0): the non-central sub-beams take
                                   the long form of the geodesy the central one takes (5 Vincenty passes, atan2 ->
                                   degrees -> sincos, correctly rounded division / square root) instead of the short
                                   form (4 passes, reciprocal roots + Newton, short series): what
                                   tests/test_gpu_fullsize.py and tools/fast_sub_check.py compare the short form with */
    double  c_spectrum;         /* wavelength^4 / (pi^5 K^2 K^2)  (doppler_scatter.py:709) */
    /* Doppler scheme 3: broadening of every sub-beam's spectrum by turbulence and antenna motion
       (doppler_scatter.py:360-369, 727-801).  All zero = off: a caller that zero-initialises the struct and knows nothing of
       these fields gets the unbroadened spectrum.  Either switch outside scheme 3, turbulence without a valid var_edr, or a
       switch with v_res <= 0 is CPOL_ERR_ARG (the context stays usable). */
    int32_t turbulence_correction;  /* 1: add spectral_width_turb(RANGE_RADAR, EDR) to the width of every gate          */
    int32_t motion_correction;      /* 1: add spectral_width_motion(elevation)                                         */
    int32_t var_edr;                /* staged-variable index of the eddy dissipation rate (read only with turbulence)  */
    int32_t terrain_shadow;         /* 0 (a zero-initialised struct): every gate of a sub-beam depends on itself alone, as in the
                                       reference.  1: TERRAIN SHADOWING -- a sub-beam stays blocked behind its first gate below the
                                       topography, see "Terrain shadowing" below.  (The slot was padding: nothing moved.)           */
    double  sigma_r;                /* 0.35 * radial_resolution [m]                                                    */
    double  sigma_theta;            /* deg2rad(3dB_beamwidth) / (4 sqrt(ln 2))                                         */
    double  motion_num;             /* (wavelength / 100) * antenna_speed -- the reference's statement, mm / 100       */
    double  motion_den;             /* 2 pi deg2rad(3dB_beamwidth)                                                     */
    double  v_res;                  /* VARRAY[2] - VARRAY[1] [m/s]: sigma in bins = width / v_res                      */
} cpol_sweep_params;

#define CPOL_DEBUG_EXACT_SUBBEAMS 1

/* ray-path models */
enum {
    CPOL_GEOM_GROUND_43 = 0,    /* 4/3-earth closed form (atm_refraction.py:181-220)    */
    CPOL_GEOM_SPACEBORNE = 1,   /* straight ray from orbit, KE = 1, gates below 35 km
                                   (atm_refraction.py:222-272, intended behaviour)      */
    CPOL_GEOM_HOST_PATHS = 2    /* (s, h, e) per gate supplied by the host, e.g. the
                                   Zeng & Blahak ODE (atm_refraction.py:79-148)          */
};

/* per-ray host-side tables (cpol_ray_tables fills them) */
typedef struct {
    const double *traj;         /* [n_rays][n_vnodes][CPOL_TRAJ_STRIDE = 4] : el_rad,
                                   sin el, cos el, el_deg                       */
    const double *geo;          /* [n_rays][n_hnodes][CPOL_GEO_STRIDE = 8] : sin a1,
                                   cos a1, sigma1, sin alpha, b*A, B, C, azimuth_rad */
    const int32_t *sub_h;       /* [n_sub] horizontal node of each kept sub-beam */
    const int32_t *sub_v;       /* [n_sub] vertical node                        */
    const double *sub_w;        /* [n_sub] quadrature weight                    */
    const double *sens_thr;     /* [n_gates] dBZ threshold per gate or NULL      */
    const double *site;         /* [n_rays][8] per-ray radar site or NULL (= the one
                                   of cpol_sweep_params): sin U1, cos U1, lon [deg],
                                   altitude [m], earth radius [m], first kept gate
                                   index, number of kept gates, unused             */
    const float *paths;         /* CPOL_GEOM_HOST_PATHS: [n_rays][n_vnodes][3][n_gates]
                                   float32 (s, h, e_deg), NaN = no gate            */
    const double *nyquist;      /* [n_rays] Nyquist velocity per ray [m/s] for the RVEL
                                   aliasing (utilities.py:142-156) or NULL (no folding) */
    uint64_t version;           /* 0: tables are uploaded on every call; otherwise the
                                   caller's tag of this table set -- a context keeps the
                                   device copies of the last 8 tags it has seen (same tag
                                   and same shapes: nothing is uploaded), so a scan that
                                   cycles through its elevations uploads each set once  */
    /* integration scheme 'ml' (interpolation.py:168-193, 423-436; per-gate weights as in
       doppler_scatter.py:124-129, 186-189, 259-264): NULL / 0 for scalar weights */
    const double *varray;       /* [n_vbins] velocity bins of the Doppler spectrum
                                   (Doppler scheme 3) or NULL                          */
    const int32_t *sub_smooth;  /* [n_sub] 1: the weight of this sub-beam is sub_w x the
                                   Gaussian-smoothed mask of the first / last melting-layer
                                   gate of the sub-beam; 0: sub_w at every gate          */
    const double *ml_filter;    /* [2 * ml_radius + 1] filter taps (scipy gaussian_filter) */
    int32_t ml_radius;
    int32_t pad_;
    /* time blend (cpol_run_sweep_members only; all zero = off: a caller that zero-initialises the struct and knows nothing of
       these fields gets the ensemble call).  Set in any other entry point that takes tables: CPOL_ERR_ARG.  They are per-ray
       tables and live here, not in cpol_sweep_params, whose last member stays v_res. */
    const int32_t *ray_state;   /* [n_rays] host: index INTO `members` of the earlier state                          */
    const float   *ray_weight;  /* [n_rays] host: weight of the later state, 0 <= w < 1; 0 = the earlier state alone */
    int32_t time_blend;         /* 1: ONE scan whose ray r reads members[ray_state[r]] blended with members[ray_state[r] + 1] */
    int32_t pad_time_;
} cpol_ray_tables_t;

/* Superobservations: what a data-assimilation system consumes instead of one value per gate -- averages of the per-gate
 * fields over windows of ray_window rays x gate_window gates, with the number of gates that went into each.  Replaces in
 * the reference: nothing (it hands back per-gate radials).  Pointed to by cpol_outputs.superob; honoured by cpol_run_sweep
 * and cpol_run_sweep_members (ensemble and time blend), refused by cpol_run_columns.
 * INPUT: the per-gate fields of the call as the launch sequence leaves them (after the range scans and the sensitivity cut;
 * censored gates are NaN): n_rows rows of n_gates gates, n_rows = n_rays, or n_members * n_rays for an ensemble call.
 * WINDOWS tile the rows in blocks of rays_per_block rows: window row i of a block holds its rays [i R, min((i + 1) R,
 * rays_per_block)), window column j the gates [j G, min((j + 1) G, n_gates)); a window never crosses a block (so it stays
 * inside one member, one sweep of a grouped scan); the last windows may be partial; no azimuth wrap-around.  n_cells =
 * (n_rows / rays_per_block) * ceil(rays_per_block / R) * ceil(n_gates / G), blocks stacked in row order, columns fastest.
 * PER FIELD: a gate counts when its value is not NaN, n = the counting gates; per ray of the window in ascending order s_r =
 * the float64 sum of its counting values in ascending gate order from +0.0; S = the float64 sum of the s_r in ascending ray
 * order from +0.0; the superobservation is S / n (float64 division), rounded once to float32 for the float32 fields; NaN when
 * n < need = max(1, (int)ceil(min_valid_fraction * N)), N = the gates the window actually holds.
 * ZDR is the ratio of the window's mean powers: over the gates where ZH and ZV both count, S_H and S_V by the rule above,
 * ZDR = (float)(S_H / S_V), n = those gates.  RVEL after aliasing: the mean of the folded velocities, nothing is unfolded.
 * mask, model_vars, sz_total and DSPECTRUM are not averaged.
 * The output pointers follow p->outputs_on_device like every other array (mode 2: they count for the one-copy window rule).
 * CPOL_ERR_ARG, nothing queued, the context usable: a window < 1, R * G > 65535 (count is uint16), min_valid_fraction outside
 * (0, 1] or NaN, rays_per_block < 0 or not dividing n_rows, none of the ten field pointers set, RVEL without Doppler.
 * ONE kernel (k_superob) runs behind the launch sequence and before the output copy: the per-gate arrays, the launch forms,
 * the gate stencils and a captured graph are what they are without it.  A per-gate array the caller leaves NULL is still
 * produced on the device (the context's own buffer) and simply not copied. */
typedef struct cpol_superob {
    int32_t ray_window;         /* R >= 1                                                                  */
    int32_t gate_window;        /* G >= 1                                                                  */
    int32_t rays_per_block;     /* 0: p->n_rays of the call; else it must divide the call's row count      */
    int32_t pad_;
    double  min_valid_fraction; /* in (0, 1]                                                               */
    /* all [n_cells]; NULL = not wanted */
    float  *ZH, *ZV, *ZDR, *KDP, *DELTA_HV, *PHIDP, *RHOHV, *ATT_H, *ATT_V;
    double *RVEL;
    uint16_t *count;            /* [10][n_cells] or NULL: n of every field, rows in the order ZH, ZV, ZDR, KDP, DELTA_HV, PHIDP,
                                   RHOHV, ATT_H, ATT_V, RVEL; only the rows of requested fields are written (mode 2 under the
                                   window rule: the other rows lie inside the window and arrive as zeros) */
} cpol_superob;

/* Ensemble statistics: what a probabilistic forecast or its verification consumes instead of every member's per-gate arrays
 * -- per gate the mean, the spread, the extremes, the number of members with an echo and the number of members above
 * thresholds.  Replaces in the reference: nothing (it runs one model state per process).  Pointed to by
 * cpol_outputs.member_stats; honoured by cpol_run_sweep (folds ONE member: the rows of the call, the context's selected
 * member) and by cpol_run_sweep_members without time blend (folds the call's n_members row sets in the order of `members`).
 * A RUNNING FOLD with state on the device, one state per context: a pass is open from a call with the begin bit until a call
 * with the finish bit or the next begin; the result does not depend on how the member list was cut into calls.
 * INPUT: the per-gate fields of the call as the launch sequence leaves them (after the range scans and the sensitivity cut;
 * censored gates are NaN).  A cell is a gate of the call, n_cells = n_rays * n_gates (n_rays of ONE member).
 * FIELDS: the ten of cpol_superob.count's rows in that order (bit k of `fields`): ZH, ZV, ZDR, KDP, DELTA_HV, PHIDP, RHOHV,
 * ATT_H, ATT_V float32, RVEL float64 (type T below).  ZDR is folded from each member's own per-gate ZDR like any other field.
 * mask, model_vars, sz_total and DSPECTRUM are not folded.
 * STATE per cell and folded field: n uint16 = 0; mean, M2 float64 = +0.0; lo, hi of type T = +inf, -inf; k_t uint16 = 0, one
 * per threshold.  Members are folded one after another, in the order of the call's member list and of the calls of the pass.
 * For a member's value v: it counts iff v == v (a NaN changes nothing).  If it counts:
 *     n = n + 1;  d = (double)v - mean;  mean = mean + d / (double)n;  M2 = M2 + d * ((double)v - mean)   (the new mean);
 *     if (v < lo) lo = v;  if (v > hi) hi = v;  k_t += (v > thr_t) for each threshold,
 * thresholds compared in type T (thr_t: the caller's double rounded once to float32 for the float32 fields); every operation
 * one IEEE operation (no contraction, no reciprocal; a subnormal quotient is rounded once too).
 * FINISHING, need = min_members >= 1: mean = (T)mean where n >= need, else NaN; spread = (T)sqrt(M2 / (double)(n - 1)) where
 * n >= max(need, 2), else NaN (the sample standard deviation); min = lo and max = hi where n >= need, else NaN; count = n and
 * exceed_t = k_t always.  Counts, not probabilities: the host divides by the members folded or by count, as it likes.
 * The output pointers are read only by a finishing call and follow p->outputs_on_device like every other array (mode 2:
 * they count for the one-copy window rule).  Pointers of a field outside `fields` are ignored.
 * CPOL_ERR_ARG, nothing queued, the state of an open pass untouched, the context usable: phase outside 0..3; min_members < 1;
 * fields zero or with a bit >= 10; RVEL without Doppler; an n_thresholds outside 0..8, or positive with a NULL pointer; a NaN
 * threshold; a fold with no pass open and no begin bit; a fold whose n_cells, fields, thresholds or min_members differ from
 * the open pass; more than 65535 members in a pass; a finishing call with no output pointer at all; outputs->superob set in
 * the same call; tables->time_blend; cpol_run_columns and cpol_interp_subbeams.
 * TWO kernels (k_member_fold, k_member_finish) run behind the launch sequence and before the output copy: the per-gate
 * arrays, the launch forms, the gate stencils and a captured graph are what they are without it.  A per-gate array the
 * caller leaves NULL is still produced on the device (the context's own buffer) and simply not copied.
 * QUANTILES (quantile_capacity > 0; a third kernel, k_member_quantile, behind k_member_finish).  Per cell and per field with
 * n_quantiles[k] > 0: the counting values of the pass (v == v, exactly the ones the fold counts; n of them) are ordered
 * ascending by <, with -0.0 before +0.0 -- a total order on everything that is not NaN, +-inf included; sorted they are
 * x[0] ... x[n-1].  For a quantile q in [0, 1]: h = q * (double)(n - 1), one IEEE multiplication.  quantile_method, one per pass:
 *     0 linear:  i = floor(h); g = h - (double)i; a = (double)x[i].  g == 0: a.  Else b = (double)x[i+1]; a == b: a.  Else
 *                r = a + g * (b - a), three separate float64 operations without contraction, then if (r > b) r = b.  The
 *                quantile is (T)r, rounded once.  An infinite bracket gives what IEEE gives: between -inf and any other
 *                value that is NaN, between a finite value and +inf it is +inf.
 *     1 lower:   x[floor(h)];   2 higher: x[ceil(h)];   3 nearest: x[rint(h)], ties to even.  A member's own bits, no trip
 *                through float64.
 * The quantile is NaN where n < need.  Because the order is total the result is a symmetric function of the members: it depends
 * neither on the order of the member list nor on how the pass is cut into calls.  The device keeps every member of a field with
 * quantiles until the pass finishes: a stash of quantile_capacity * n_cells * sizeof(T) bytes per such field, owned by the
 * context, sized when the pass begins and freed with the context.  A pass with quantiles holds at most quantile_capacity <= 128
 * members; the other statistics keep their limit of 65535.  The quantile lists of a field that is not folded are not read.
 * CPOL_ERR_ARG in addition, on the same terms: quantile_method outside 0..3; quantile_capacity outside 0..128; quantiles with
 * capacity 0; an n_quantiles outside 0..8, or positive with a NULL array; a q that is NaN or outside [0, 1]; a fold whose
 * capacity, method or quantile lists differ from the open pass; a call that would take a pass with quantiles beyond its
 * capacity.  A finishing call whose only output pointers are quantile pointers is a valid finishing call. */
#define CPOL_MEMBER_STATS_FIELDS 10
#define CPOL_MEMBER_STATS_MAX_THRESHOLDS 8
#define CPOL_MEMBER_STATS_MAX_QUANTILES 8
#define CPOL_MEMBER_STATS_MAX_QUANTILE_MEMBERS 128
typedef struct cpol_member_stats {
    int32_t phase;              /* bit 0: begin a pass (clear the state, then fold); bit 1: finish it (fold, then write the
                                   outputs); 0: fold only                                                          */
    int32_t min_members;        /* need >= 1                                                                       */
    uint32_t fields;            /* bit k: fold field k                                                             */
    int32_t n_thresholds[CPOL_MEMBER_STATS_FIELDS];     /* 0..8 per field                                          */
    int32_t pad_;
    const double *thresholds[CPOL_MEMBER_STATS_FIELDS]; /* host arrays [n_thresholds[k]], the field's own (linear) units */
    /* outputs, each [n_cells], float32 except slot RVEL (float64); NULL = not wanted */
    void *mean[CPOL_MEMBER_STATS_FIELDS], *spread[CPOL_MEMBER_STATS_FIELDS];
    void *min[CPOL_MEMBER_STATS_FIELDS], *max[CPOL_MEMBER_STATS_FIELDS];
    uint16_t *count;            /* [10][n_cells] or NULL: n of every field; only the rows of folded fields are written (mode 2
                                   under the window rule: the other rows arrive as zeros)                          */
    uint16_t *exceed[CPOL_MEMBER_STATS_FIELDS];         /* [n_thresholds[k]][n_cells] or NULL                      */
    /* quantiles: appended, so that nothing above moves and a zero-initialised struct has none */
    int32_t quantile_capacity;  /* 0: no quantiles.  Else the members this pass may hold, 1..128; the stash is sized by it
                                   when the pass begins                                                            */
    int32_t quantile_method;    /* 0 linear, 1 lower, 2 higher, 3 nearest                                          */
    int32_t n_quantiles[CPOL_MEMBER_STATS_FIELDS];      /* 0..8 per field                                          */
    const double *quantiles[CPOL_MEMBER_STATS_FIELDS];  /* host arrays [n_quantiles[k]], each in [0, 1]            */
    void *quantile[CPOL_MEMBER_STATS_FIELDS];           /* outputs [n_quantiles[k]][n_cells], float32 (slot RVEL float64);
                                                           NULL = not wanted; read by a finishing call             */
} cpol_member_stats;

/* Spectrum moments: what a user of a Doppler radar simulation compares with a radar instead of the spectrum itself -- per gate
 * the power, the mean velocity, the spectrum width, skewness and kurtosis, the peak and the edges of the gate's Doppler spectrum
 * AS THE CALL DELIVERS IT.  Replaces in the reference: nothing (it forms no moment of the spectrum but RVEL).  Pointed to by
 * cpol_outputs.spectrum_moments; honoured by cpol_run_sweep with simulate_doppler == 3.
 * INPUT per gate: the row S[0 .. n_v-1] of DSPECTRUM as k_spec_final leaves it, float64 -- after the sub-beam accumulation and
 * after the bin-by-bin sensitivity cut, so censored bins are NaN -- and V[v], the caller's float64 varray.  The gate-level ZH
 * censoring of the other observables is NOT applied and nothing is folded into the Nyquist interval: the result is what the
 * rule below gives on the host for the delivered DSPECTRUM.
 * COUNTING: a bin counts iff S[v] == S[v] && S[v] > min_power (min_power >= 0, finite, linear units); n = the counting bins.
 * ORDERED SUM R[t] of a per-bin term t, float64, every operation one IEEE operation (no contraction, no reciprocal):
 *     for lane l = 0 .. 63: a_l = +0.0; then for v = l, l + 64, l + 128, ... ascending below n_v, if bin v counts:
 *     a_l = a_l + t[v]; then for off = 32, 16, 8, 4, 2, 1: every lane at once a_l = a_l + a_(l xor off); R[t] = a_0 (all lanes
 *     hold the same value).
 * PASS 1: P = R[S]; M = R[V * S] (the product formed first, then added); vbar = M / P.
 * PASS 2, per counting bin d = V[v] - vbar, d2 = d * d: C2 = R[d2 * S]; C3 = R[(d2 * d) * S]; C4 = R[(d2 * d2) * S].
 * FINISHING: var = C2 / P; WIDTH = sqrt(var); SKEWNESS = (C3 / P) / (var * WIDTH); KURTOSIS = (C4 / P) / (var * var);
 * POWER = P; VMEAN = vbar; VPEAK = V[i], i the lowest index among the counting bins that hold the largest S; VLOW = V[lowest
 * counting index]; VHIGH = V[highest counting index].  Every field is NaN where n < min_bins; count = n always (uint16).
 * Not special-cased: n == 1 gives WIDTH = 0 and NaN for skewness and kurtosis; overflow gives the inf or NaN IEEE gives.
 * ROWS of `moments` (bit k of `fields`): POWER, VMEAN, WIDTH, SKEWNESS, KURTOSIS, VPEAK, VLOW, VHIGH.
 * The output pointers follow p->outputs_on_device like every other array (mode 2: they count for the one-copy window rule; rows
 * of `moments` outside `fields` that lie inside the window arrive as zeros).
 * CPOL_ERR_ARG, nothing queued, the context usable: the struct set outside Doppler scheme 3; fields zero or with a bit >= 8;
 * min_bins < 1 or > 65535; min_power negative, NaN or infinite; moments NULL; outputs->superob or outputs->member_stats set in
 * the same call; cpol_run_sweep_members and cpol_run_columns.
 * ONE kernel (k_spec_moments, one wavefront per gate) runs behind the launch sequence and before the output copy: the per-gate
 * arrays, the launch forms, the gate stencils and a captured graph are what they are without it.  When the caller leaves
 * DSPECTRUM NULL the spectrum is still produced on the device (the context's own buffer) and simply not copied. */
#define CPOL_SPECTRUM_MOMENTS_FIELDS 8
typedef struct cpol_spectrum_moments {
    uint32_t fields;            /* bit k: row k wanted                                                             */
    int32_t  min_bins;          /* need >= 1                                                                       */
    double   min_power;         /* >= 0, finite                                                                    */
    double  *moments;           /* [8][n_rays * n_gates]; only the rows in `fields` are the caller's to be written */
    uint16_t *count;            /* [n_rays * n_gates] or NULL                                                      */
} cpol_spectrum_moments;

/* Ensemble verification: the members of a pass of ensemble statistics scored against an observation per gate -- the rank of the
 * observation among the members and the CRPS.  Replaces in the reference: nothing.  Pointed to by cpol_outputs.member_verify;
 * honoured by cpol_run_sweep and cpol_run_sweep_members, together with cpol_outputs.member_stats only.
 * THE RULE (the same text stands in cosmo_pol_amd/ensemble_verify.py).  A cell is a gate of the call.  A verified field k is one of
 * the ten of cpol_member_stats, bit k of `fields`; its type T is float32, except RVEL, which is float64.  Each verified field has
 * an observation array obs[k] of n_cells values of type T; the observation y = obs[k][c] is in the field's own (linear) units; NaN
 * means no observation.  The counting members of the pass are exactly the ones the fold counts (v == v, n of them), ordered by the
 * total order of the quantile rule (-0.0 before +0.0, +-inf included; key() below is that order as an integer); sorted they are
 * x[0] ... x[n-1].
 * RANKS: below = the number of i with key(x[i]) < key(y); equal = the number of i with key(x[i]) == key(y).  Both uint16, both
 * written always, like `count`, and both 0 where y is NaN.  min_members does not gate them.
 * CRPS (type T): NaN where y is NaN; NaN where n < need (min_members); NaN where n == 0; with `fair`, NaN where n < 2.  Otherwise
 * in float64, every operation one IEEE operation, no contraction and no reciprocal:
 *     yd = (double)y;
 *     A = +0.0; for i = 0 ... n-1 ascending: A = A + fabs((double)x[i] - yd);
 *     B = +0.0; for i = 0 ... n-1 ascending: B = B + (double)(2*i - n + 1) * (double)x[i]   (the product formed first, then added);
 *     D = n*n, or n*(n-1) when `fair` (a whole number of at most 16384);
 *     r = A / (double)n - B / (double)D   (each quotient rounded once, subnormal quotients too);
 *     if (r < 0) r = +0.0;  crps = (T)r.
 * This is (1/n) sum |x_i - y| - (1/2D) sum_i sum_j |x_i - x_j|: the double sum over ordered pairs is 2B for a sorted sample.
 * Infinite members or observations are not special-cased: IEEE decides.  The sums run over the sorted values, so all three outputs
 * are symmetric functions of the members: they depend neither on the order of the member list nor on how the pass is cut into calls.
 * A verified field keeps its members like a field with quantiles: one stash per field (shared with its quantiles if it has any),
 * sized by member_stats->quantile_capacity when the pass begins; a pass with a verified field holds at most that many (<= 128)
 * members.  The struct accompanies EVERY call of the pass with the same `fields` and `fair`; obs and the output pointers are read
 * by the finishing call only.  obs[k] lies where the outputs lie: with p->outputs_on_device == 0 a host array (copied to a buffer
 * of the context on the call's stream), in modes 1 and 2 an array the device reads in place (device memory, or page-locked memory of
 * cpol_host_alloc).  The outputs follow p->outputs_on_device like the other statistics arrays (mode 2: they count for the window rule).
 * ONE kernel (k_member_verify) runs behind k_member_quantile in a finishing call, before the output copy.  A pass without the
 * struct queues what it queued without it.
 * CPOL_ERR_ARG, nothing queued, an open pass untouched, the context usable: member_verify without member_stats; fields zero, with a
 * bit >= 10 or with a bit outside member_stats->fields; fair outside 0 / 1; quantile_capacity == 0; a fold that would exceed the
 * capacity; a call that does not begin a pass whose fields or fair differ from the open pass, or that presents the struct to a pass
 * begun without it; a call of a pass begun with the struct that leaves it out; a finishing call with a verified field whose obs is
 * NULL or that has no verify output pointer at all; outputs->superob in the same call; cpol_run_columns, cpol_interp_subbeams and
 * time-blended calls. */
typedef struct cpol_member_verify {
    uint32_t fields;            /* bit k: verify field k (a subset of member_stats->fields); 0 verifies nothing and is refused */
    int32_t fair;               /* 0: D = n*n; 1: D = n*(n-1)                                                      */
    const void *obs[CPOL_MEMBER_STATS_FIELDS];      /* [n_cells] float32 (slot RVEL float64); NaN = no observation */
    uint16_t *below[CPOL_MEMBER_STATS_FIELDS];      /* outputs [n_cells]; NULL = not wanted                        */
    uint16_t *equal[CPOL_MEMBER_STATS_FIELDS];
    void *crps[CPOL_MEMBER_STATS_FIELDS];           /* [n_cells] float32 (slot RVEL float64)                       */
} cpol_member_verify;

/* Sweep histograms: CFADs, joint counts and plain histograms of the per-gate fields of a call, counted on the device, for the
 * user who wants a DISTRIBUTION over many gates instead of one value per gate.  Replaces in the reference: nothing (its users
 * pull every per-gate array to the host and call np.histogram2d there).  Pointed to by cpol_outputs.histogram; honoured by
 * cpol_run_sweep and cpol_run_sweep_members (the ensemble and the time blend).  cosmo_pol_amd/histogram.py states the same rule
 * in NumPy (`count`).
 * INPUT: the per-gate fields of the call as the launch sequence leaves them: after the range scans and the sensitivity cut,
 * censored gates NaN; n_rows rows of n_gates gates (n_rows = n_rays, or n_members * n_rays in an ensemble call).
 * FIELDS: the ten of cpol_superob.count's rows, in that order.  The type T is float32, except RVEL: float64.
 * ABSCISSA: field k has n_x[k] >= 1 bins between n_x[k] + 1 edges.  The caller gives the edges as float64 in the field's own
 * linear units; they are rounded once to T and must then be finite and strictly ascending.  The bin of a value v is
 * ix = #{ j : e[j] <= v }, compared in T, in 0 ... n_x + 1: bin 0 is underflow, bin n_x + 1 overflow.  This is
 * np.searchsorted(e_T, v, side='right'): comparisons only, no arithmetic, so the device cannot differ from NumPy.  +-inf land in
 * the outer bins by themselves; -0.0 on an edge at +0.0 lands at or above it, as IEEE <= says.
 * ORDINATE, optional, one per struct: code 0 none (1-D); 1 `heights` (float32); 2 `dist` (float32); 16 + k field k (its type);
 * 32 + v row v of `model_vars` (float64; only where the call produces model_vars: a CFAD by temperature).  n_y >= 1 bins, n_y + 1
 * edges, the same rule: iy in 0 ... n_y + 1.  In an ensemble call without time blend the geometry arrays hold n_rays rows once:
 * row r takes the ordinate of row r mod n_rays.
 * COUNTING: a gate counts for field k iff v == v, and with an ordinate also y == y; a counting gate adds 1 to
 * counts[k][block][iy][ix].
 * BLOCKS: rays_per_block = 0 gives one histogram for all rows of the call.  Otherwise it must divide n_rows, and block b holds
 * the rows [b * rpb, (b + 1) * rpb): rpb = n_rays one histogram per member, rpb = 1 one per ray.
 * COUNTS: uint64, [n_blocks][n_y + 2][n_x[k] + 2], or [n_blocks][n_x[k] + 2] without an ordinate.
 * A RUNNING PASS, like cpol_member_stats.phase: bit 0 begins (clears, then counts), bit 1 finishes (counts, then writes out), 0
 * only counts.  The state is one per context, lives on the device and holds the counts themselves.  The calls of a pass may have
 * different n_rays, n_gates and geometry when rays_per_block == 0 (a volume's sweeps, a year of model states fold into one CFAD);
 * with rays_per_block > 0 every call must give the same number of blocks.  The result is a sum of integers: it depends neither
 * on how the pass is cut into calls nor on any order of addition.
 * LIMITS (conditions, not measurements): n_x[k] + 1 and n_y + 1 at most 1024; (n_x[k] + 2) * (n_y + 2) at most 16 384 cells per
 * field (one field's table fits 64 KiB of LDS as uint32); n_blocks * sum_k cells_k at most 2^27 (1 GiB of state).
 * The counts pointers follow p->outputs_on_device like every other array (mode 2: they count for the one-copy window rule); they
 * are read by a finishing call only.
 * CPOL_ERR_ARG, nothing queued, an open pass untouched, the context usable: phase outside 0..3; fields zero or with a bit >= 10;
 * RVEL, as field or ordinate, without Doppler; an unknown ordinate code; ordinate 32 + v when the call makes no model_vars, or
 * with v >= n_vars; an ordinate set while n_y < 1 or edges_y is NULL; n_y != 0 with ordinate 0; an n_x of a requested field < 1
 * or over the limit; a NULL edge array; an edge that is NaN or infinite; edges not strictly ascending AFTER ROUNDING TO T; any
 * of the three limits exceeded; rays_per_block < 0 or not dividing n_rows; a counting call with no pass open and no begin bit; a
 * call whose fields, edges, ordinate or block count differ from the open pass; a finishing call with no counts pointer for any
 * requested field; outputs->superob, member_stats or spectrum_moments in the same call; cpol_run_columns and
 * cpol_interp_subbeams.
 * ONE kernel per requested field (k_hist, cpol_hist.inl) runs behind the launch sequence and before the output copy: the
 * per-gate arrays, the launch forms, the gate stencils and a captured graph are what they are without it.  A per-gate array the
 * caller leaves NULL is still produced on the device and is not copied.  With ordinate 32 + v the call produces model_vars as
 * if the caller had asked for them (p->integrate_model must be set). */
#define CPOL_HIST_FIELDS 10
typedef struct cpol_histogram {
    uint32_t fields;            /* bit k: field k counted                                                          */
    int32_t  phase;             /* bit 0 begins the pass, bit 1 finishes it                                        */
    int32_t  ordinate;          /* 0 none, 1 heights, 2 dist, 16 + k field k, 32 + v row v of model_vars           */
    int32_t  n_y;               /* bins of the ordinate (0 without one)                                            */
    int32_t  rays_per_block;    /* 0: one block of all rows; else divides the rows of the call                     */
    int32_t  n_x[CPOL_HIST_FIELDS];             /* bins of field k's abscissa                                      */
    const double *edges_x[CPOL_HIST_FIELDS];    /* [n_x[k] + 1], the field's own linear units                      */
    const double *edges_y;                      /* [n_y + 1] or NULL                                               */
    uint64_t *counts[CPOL_HIST_FIELDS];         /* [n_blocks][n_y + 2][n_x[k] + 2]; read by a finishing call        */
} cpol_histogram;

/* Gridded composites: the column maximum, the lowest gate and echo-top heights of the per-gate fields of a call on a
 * radar-centred map, reduced on the device, for the user who wants a MAP instead of one value per gate.  Replaces in the
 * reference: nothing (its users pull every per-gate array to the host, compute per gate where it lies and scatter with
 * np.maximum.at).  Pointed to by cpol_outputs.composite; honoured by cpol_run_sweep and cpol_run_sweep_members (the ensemble and
 * the time blend).  cosmo_pol_amd/composite.py states the same rule in NumPy (`compose`, `finish`).
 * INPUT: the per-gate fields of the call as the launch sequence leaves them: after the range scans and the sensitivity cut,
 * censored gates NaN; n_rows rows of n_gates gates (n_rows = n_rays, or n_members * n_rays in an ensemble call).  With them
 * `dist` (float32, ground distance of the central sub-beam) and `heights` (float32) of the same call, and per ray two float64
 * numbers ray_sin[r], ray_cos[r] GIVEN BY THE CALLER (the Python layer: np.sin(np.deg2rad(az)), np.cos(np.deg2rad(az))): the
 * library computes no trigonometric function for this product, so the device and the rule cannot differ there.  Geometry arrays
 * that hold n_rays rows once (an ensemble call without time blend) are read at g mod (n_rays * n_gates), the per-ray pair at
 * row mod n_rays.
 * PLANE: radar-centred, east x and north y: x = (double)dist * ray_sin, y = (double)dist * ray_cos -- ONE float64
 * multiplication each (the library is built with -ffp-contract=off).
 * GRID: n_x + 1 and n_y + 1 float64 edges, finite and strictly ascending, at most 1024 per axis.  ix = #{ j : ex[j] <= x } - 1,
 * likewise iy: comparisons alone, np.searchsorted(e, x, side='right') - 1.  The gate lies in the grid iff 0 <= ix < n_x and
 * 0 <= iy < n_y: there are no under- or overflow cells (a gate on the last edge is outside), and a gate outside does not count.
 * HEIGHT SLAB, optional (use_slab): [h_lo, h_hi), both bounds rounded once to float32, the test h_lo <= h && h < h_hi in
 * float32.  Without a slab every height counts.
 * FIELDS: the nine float32 fields ZH ... ATT_V, bit k as in cpol_histogram.fields.  RVEL (float64) is refused.
 * COUNTING: a gate counts for field k iff v == v, dist == dist, h == h, it lies in the grid and it lies in the slab.
 * THE ORDERED KEY of a float32 with bits b: key = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000), a total order
 * -inf < ... < -0.0 < +0.0 < ... < +inf.  Keys 0 and 0xFFFFFFFF belong to NaN bit patterns: no counting value produces them,
 * and they mark an empty cell.
 * PRODUCTS per requested field, a bit mask, the same for all fields of a struct:
 *   CPOL_COMP_MAX      `max`, `height_of_max`: one uint64 per cell, the MAXIMUM of key(v) << 32 | key(h) over the counting
 *                      gates; ties in the value go to the greater height.
 *   CPOL_COMP_LOWEST   `lowest`, `height_of_lowest`: one uint64 per cell, the MINIMUM of key(h) << 32 | key(v); ties in the
 *                      height go to the smaller value.
 *   CPOL_COMP_ECHO_TOP `echo_top_0` ... : n_thresholds[k] in 1 ... 4 planes for field k, thresholds in the field's own linear
 *                      units, each rounded once to float32 (not NaN); per plane one uint32 per cell, the maximum of key(h) over
 *                      the counting gates with v >= t.  Without this bit every n_thresholds must be 0.
 *   `count` is always produced: uint64 per cell and field, the number of counting gates.
 * BLOCKS AND PASS, exactly as in cpol_histogram: rays_per_block = 0 one map of all rows, else it divides n_rows (n_rays: one map
 * per member).  phase bit 0 begins (max states 0, min states all ones, counts 0), bit 1 finishes.  The state is one per context,
 * on the device.  With rays_per_block == 0 the calls of a pass may differ in n_rays, n_gates and geometry: the sweeps of a volume
 * fold into one composite.  Every result is a max, a min or a sum of integers: it depends neither on how the pass is cut into
 * calls nor on any order.
 * OUTPUTS, read by a finishing call only: per requested field one float32 array values[k], [n_blocks][n_planes][n_y][n_x], the
 * planes in the fixed order max, height_of_max, lowest, height_of_lowest, echo_top_0 ..., planes not requested absent, empty
 * cells NaN; one uint64 array count, [n_blocks][n_requested_fields][n_y][n_x], the fields ascending.  The pointers follow
 * p->outputs_on_device like every other array.
 * LIMITS (conditions, not measurements): at most 1024 edges per axis; the state of all blocks and fields at most 1 GiB; fewer
 * than 2^31 workgroups.
 * CPOL_ERR_ARG, nothing queued, an open pass untouched, the context usable: phase outside 0..3; fields zero or with a bit >= 9
 * (RVEL); products zero or with an unknown bit; n_thresholds outside 1..4 with ECHO_TOP or non-zero without; a NaN threshold;
 * a slab with h_lo >= h_hi after rounding (or a NaN bound); n_x or n_y < 1 or over the limit; a NULL edge array; an edge NaN or
 * infinite; edges not strictly ascending; a limit exceeded; rays_per_block < 0 or not dividing n_rows; NULL ray_sin or ray_cos; a
 * counting call with no pass open and no begin bit; a call whose fields, products, thresholds, slab, edges or block count differ
 * from the open pass; a finishing call without `count` or without `values` of a requested field; a spaceborne call (per-ray
 * radar positions: tables->site); outputs->superob, histogram, member_stats or spectrum_moments in the same call;
 * cpol_run_columns and cpol_interp_subbeams.
 * ONE kernel per requested field (k_comp, cpol_comp.inl) runs behind the launch sequence and before the output copy, and a
 * finishing call adds k_comp_finish per field: the per-gate arrays, the launch forms, the gate stencils and a captured graph are
 * what they are without it.  A per-gate array the caller leaves NULL is still produced on the device and is not copied.
 *
 * NETWORK COMPOSITES: several radars on one geographic or model grid.  Everything above stays as it is; a zero-initialised new
 * member means the behaviour above.
 * PLANE (`plane`): CPOL_COMP_PLANE_RADAR = 0 is the radar-centred plane above.  With CPOL_COMP_PLANE_GATES = 1 the caller
 * supplies per-gate coordinates, const double gate_x[geo_rays * n_gates], gate_y[geo_rays * n_gates], read at g mod geo_gates
 * exactly as `dist` is: x = gate_x[g], y = gate_y[g], no multiplication.  ray_sin / ray_cos may be NULL and `dist` is not read.
 * A gate counts iff v == v, h == h, x == x, y == y, it lies in the grid and it lies in the slab; the cell search is the same
 * comparisons alone.  The library still computes no trigonometric function for this product: every projection (longitude and
 * latitude, a rotated model grid, any map projection) is made by the caller.  gate_x / gate_y lie where the caller's outputs
 * lie: with outputs_on_device == 1 device memory that the device reads in place, else (0, and 2: page-locked host outputs) host
 * arrays that the library copies on the call's stream before the call returns.
 * `plane_version`: a non-zero value tells the library to keep its device copy of the two arrays under that tag and to skip the
 * upload when it holds the tag already (the idiom of cpol_ray_tables_t.version: the caller changes the tag when the arrays
 * change).  The copies are kept per context, at least as many as table sets, so the radars of a network alternating in one
 * pass do not evict each other.  cpol_debug_read "composite_plane" returns int64 {uploads, hits}.
 * SOURCE (`source`, 0 ... 254, and the product bit CPOL_COMP_SOURCE = 16, which needs MAX or LOWEST; bit 8 stays refused as an
 * unknown bit, as it always was): a number the caller gives
 * each call, e.g. the index of the radar.  New plane `source_of_max`: the smallest `source` among the counting gates of the
 * whole pass whose key(v) << 32 | key(h) equals the cell's final MAX state; `source_of_lowest`: the same for the LOWEST state.
 * Both are delivered as float32 (exact small integers), empty cells NaN.  Plane order: max, height_of_max, source_of_max,
 * lowest, height_of_lowest, source_of_lowest, echo_top_0 ....  The definition is symmetric in the calls: the pass still depends
 * neither on how it is cut into calls nor on their order.  The running state gains one source byte per cell, block and product
 * (begin value 255) and a per-call scratch state of the layout and begin values of the running state: a call of a SOURCE pass
 * composes into the scratch (k_comp, unchanged) and k_comp_merge folds it into the running state (greater: take state and
 * source; equal and not empty: the smaller source; counts add, echo tops take the maximum) and leaves the scratch at its begin
 * values.  A pass without SOURCE queues exactly what it queued before.
 * CPOL_ERR_ARG in addition, nothing queued, an open pass untouched, the context usable: `plane` outside 0 / 1; PLANE_GATES
 * with a NULL gate_x or gate_y (NULL ray_sin / ray_cos is refused on the radar plane alone); `source` outside 0 ... 254; a
 * non-zero `source` without the SOURCE bit; SOURCE without MAX and without LOWEST; `plane` differing from the open pass (the
 * SOURCE bit is part of `products`); the 1 GiB limit, which counts the source bytes and the scratch.
 *
 * HEIGHT LAYERS AND THE COLUMN: a stack of CAPPIs in one pass, and column integrals such as VIL.  Everything above stays as it
 * is; the new members lie at the end of the struct and a zero-initialised tail means off.
 * LAYERS (`n_z` = 1 ... 64, `edges_z`: n_z + 1 heights in metres, float64, each rounded once to float32 by the library; strictly
 * ascending after the rounding and not NaN).  A gate that counts above counts in layer l iff ez[l] <= h && h < ez[l + 1] in
 * float32: a gate on the last edge is outside, as on the x and y axes, and a gate below the first edge or at or above the last
 * counts nowhere.  Per (block, layer, cell) the state is the MAX state and the count of above: a block of the state holds
 * n_z * cells entries, the cell index iz * cells + iy * n_x + ix.  values[k] is float32 [n_blocks][n_z][2][n_y][n_x] (max,
 * height_of_max per layer), count uint64 [n_blocks][n_z][n_requested_fields][n_y][n_x].  With layers use_slab, LOWEST, ECHO_TOP
 * and SOURCE are refused (the first and last edge are the slab); a gate plane and several radars in one pass work as before,
 * `source` stays 0.  cpol_fractions beside a layered composite is refused.
 * COLUMN (the product bit CPOL_COMP_COLUMN = 64; it needs layers and MAX; bits 8 and 32 stay refused as unknown bits).  Per
 * requested field k an optional table: n_table[k] = 2 ... 1024 breakpoints table_v[k] (float32, in the field's linear units,
 * finite, strictly ascending) and values table_f[k] (float64, finite); n_table[k] = 0: no column of that field; at least one
 * requested field has a table.  For a layer whose maximum v exists: i = #{ j : tv[j] <= v } - 1; i < 0: f = 0.0; i >= n - 1:
 * f = tf[n - 1] (the cap; +inf takes it); else t = ((double)v - (double)tv[i]) / ((double)tv[i + 1] - (double)tv[i]),
 * f = tf[i] + t * (tf[i + 1] - tf[i]) -- every operation ONE float64 operation (-ffp-contract=off).  The column of a cell is
 * C = sum over l ascending, from +0.0, of f_l * dz_l with dz_l = (double)ez[l + 1] - (double)ez[l]: one thread adds at most 64
 * terms in a fixed order, so the result is the NumPy rule's (composite.column_of) bit for bit.  `gaps`: CPOL_COMP_GAPS_ZERO = 0 an
 * empty layer adds nothing; CPOL_COMP_GAPS_HOLD = 1 an empty layer with a counting layer below it and a counting layer above it
 * in the same cell takes the f of the nearest counting layer below; empty layers below the lowest or above the highest counting
 * layer add nothing.  A cell with no counting layer is NaN.  OUTPUTS of a finishing call: column[k] float64 [n_blocks][n_y][n_x]
 * and column_layers[k] uint8 [n_blocks][n_y][n_x] (the layers that contributed, held ones included) for every field with a
 * table; they follow p->outputs_on_device.  edges_z, table_v and table_f are host arrays, read by every call of the pass.
 * k_comp<.., LAYERS = true> composes, k_comp_finish decodes n_blocks * n_z blocks, k_comp_column (one thread per block and
 * cell, once per field with a table) integrates behind it.
 * CPOL_ERR_ARG in addition: n_z outside 0 ... 64; n_z > 0 with a NULL edges_z, a NaN edge, edges not strictly ascending after
 * the rounding, use_slab, LOWEST, ECHO_TOP or SOURCE; COLUMN without layers or without MAX; gaps outside 0 / 1, or non-zero
 * without COLUMN; n_table[k] non-zero without COLUMN or for a field not requested; n_table[k] outside 2 ... 1024; a NULL table;
 * a breakpoint or value NaN or infinite; breakpoints not strictly ascending; COLUMN with no table at all; layers, tables or gaps
 * differing from the open pass; a finishing call with a NULL column or column_layers of a field with a table; the 1 GiB limit,
 * which counts n_blocks * n_z * cells per MAX state and count.
 *
 * SUM (the product bit CPOL_COMP_SUM = 256 and the struct cpol_composite_sums below; bits 8, 32 and 128 stay refused as unknown
 * bits): the exact sum of the counting gates' weights per (block, layer, cell), for the cell MEAN and for rain accumulations.
 * Everything above stays as it is; cpol_outputs.composite points at the member `c` of a cpol_composite_sums, and the library
 * reads beyond `c` only when c.products carries the bit.  cosmo_pol_amd/composite.py states the same rule.
 *   1. A gate counts for field k exactly as above: the same cell search, slab, layers, blocks and pass.
 *   2. The summand of a counting gate is w = v when field k has no weight table (n_weight[k] == 0).  With a table (weight_v[k]
 *      float32, weight_f[k] float64) it is w = float32(f(v)), f the piecewise-linear function of the column table above: 0 below
 *      the table, the last value at and above its end, every operation one float64 operation, then ONE rounding to float32
 *      (obj_weight in cpol_obj.h, objects.weight_of).  The table conditions are those of the column table: 2 ... 1024
 *      breakpoints, finite, strictly ascending in float32, finite values; no monotonicity is demanded of the values.
 *   3. Per (block, layer, cell) `sum` is the EXACT sum of the finite w, rounded ONCE to float64 with ties to even: math.fsum of
 *      the summands.  +0.0 when the exact sum is zero, NaN when no gate was summed.
 *   4. Per (block, layer, cell) `sum_skipped` (uint32) is the number of counting gates with w = +-inf.  Such a gate is not
 *      summed, and it still counts in `count`.
 *   5. The mean is sum / (count - sum_skipped): one float64 division, formed on the host (composite.mean_of), NaN where the
 *      divisor is 0.
 *   6. Nothing depends on the order of the gates, the lane form, the block cut or how the pass is cut into calls.
 * HOW: a finite float32 is +-M * 2^(E - 150) with E in 1 ... 254 and M < 2^24 (cpol_obj.h).  The state gains per requested field
 * and (block, layer, cell) a row of 32 signed 64-bit bins and one uint32 skipped word, zeroed by a begin; bin E >> 3 takes
 * +-M << (E & 7) by a 64-bit INTEGER atomic add (k_comp_sum, one launch per field behind k_comp), and a finishing call rounds each
 * row once (k_comp_sum_finish, obj_sum_round).  Integer additions commute: no order of the hardware enters.
 * NO OVERFLOW (a condition, not a measurement): a term is below 2^31 in magnitude, so a bin cannot wrap while fewer than 2^32
 * gates fold into one block of a pass.  The library keeps the gates folded per block (rows_per_block * n_gates per call, n_rows *
 * n_gates with rays_per_block == 0) and refuses the call that would take them beyond 2^32 - 1, with nothing queued and the pass
 * untouched.
 * SUM stands beside at least one of MAX, LOWEST, ECHO_TOP (products = 256 alone is refused); SUM with SOURCE is refused; SUM with
 * layers gives a 3-D grid of sums.  COLUMN, a gate plane, several radars in one pass, blocks per member and a cpol_fractions
 * beside it work as before; the planes of values[k] do not change, so the scored plane cannot be the sum.
 * CPOL_ERR_ARG in addition: SUM alone; SUM with SOURCE; n_weight[k] non-zero for a field not requested; n_weight[k] outside
 * 2 ... 1024; a NULL table; a breakpoint or value NaN or infinite; breakpoints not strictly ascending; weight tables differing
 * from the open pass; a finishing call with a NULL sum or sum_skipped of a requested field; the 1 GiB limit, which counts the
 * bins and the skipped words; the 2^32 - 1 gates per block of a pass.
 * NOT BUILT: SUM alone, SUM with SOURCE, sums of RVEL, means in dB, a carry-normalising kernel for passes beyond 2^32 gates. */
#define CPOL_COMP_FIELDS 9
#define CPOL_COMP_MAX_THRESHOLDS 4
enum { CPOL_COMP_MAX = 1, CPOL_COMP_LOWEST = 2, CPOL_COMP_ECHO_TOP = 4, CPOL_COMP_SOURCE = 16, CPOL_COMP_COLUMN = 64,
       CPOL_COMP_SUM = 256 };                       /* (8, 32 and 128 are no products: refused) */
#define CPOL_COMP_MAX_LAYERS 64
#define CPOL_COMP_MAX_TABLE 1024
enum { CPOL_COMP_GAPS_ZERO = 0, CPOL_COMP_GAPS_HOLD = 1 };
enum { CPOL_COMP_PLANE_RADAR = 0, CPOL_COMP_PLANE_GATES = 1 };
typedef struct cpol_composite {
    uint32_t fields;            /* bit k: field k composed                                                         */
    int32_t  phase;             /* bit 0 begins the pass, bit 1 finishes it                                        */
    uint32_t products;          /* CPOL_COMP_MAX | CPOL_COMP_LOWEST | CPOL_COMP_ECHO_TOP | CPOL_COMP_SOURCE        */
    int32_t  rays_per_block;    /* 0: one block of all rows; else divides the rows of the call                     */
    int32_t  n_x, n_y;          /* cells east and north                                                            */
    int32_t  use_slab;          /* 0: every height counts; else [h_lo, h_hi)                                       */
    int32_t  n_thresholds[CPOL_COMP_FIELDS];    /* echo-top planes of field k                                      */
    double   h_lo, h_hi;        /* rounded once to float32                                                         */
    double   thresholds[CPOL_COMP_FIELDS][CPOL_COMP_MAX_THRESHOLDS];    /* the field's own linear units            */
    const double *edges_x, *edges_y;            /* [n_x + 1], [n_y + 1]                                            */
    const double *ray_sin, *ray_cos;            /* [n_rays]: sine and cosine of each ray's azimuth                 */
    float    *values[CPOL_COMP_FIELDS];         /* [n_blocks][n_planes][n_y][n_x]; read by a finishing call        */
    uint64_t *count;                            /* [n_blocks][n_requested_fields][n_y][n_x]; likewise              */
    int32_t  plane;             /* CPOL_COMP_PLANE_RADAR (0) or CPOL_COMP_PLANE_GATES                              */
    int32_t  source;            /* 0 ... 254: this call's number in the source_of_* planes (CPOL_COMP_SOURCE)      */
    const double *gate_x, *gate_y;              /* PLANE_GATES: [geo_rays * n_gates], the caller's projection      */
    uint64_t plane_version;     /* non-zero: the tag under which the library keeps gate_x / gate_y on the device   */
    int32_t  n_z;               /* 0: no height layers; else 1 ... 64 layers                                       */
    int32_t  gaps;              /* CPOL_COMP_GAPS_ZERO (0) or CPOL_COMP_GAPS_HOLD: an empty layer in the column    */
    const double *edges_z;      /* [n_z + 1] metres, each rounded once to float32                                  */
    int32_t  n_table[CPOL_COMP_FIELDS];         /* breakpoints of field k's column table; 0: no column of field k  */
    const float  *table_v[CPOL_COMP_FIELDS];    /* [n_table[k]] breakpoints in the field's linear units            */
    const double *table_f[CPOL_COMP_FIELDS];    /* [n_table[k]] values at the breakpoints                          */
    double   *column[CPOL_COMP_FIELDS];         /* [n_blocks][n_y][n_x]; read by a finishing call                  */
    uint8_t  *column_layers[CPOL_COMP_FIELDS];  /* [n_blocks][n_y][n_x]; likewise                                  */
} cpol_composite;

/* SUM (above): cpol_outputs.composite points at `c`; the library reads beyond it only when c.products carries CPOL_COMP_SUM. */
typedef struct cpol_composite_sums {
    cpol_composite c;                               /* c.products carries CPOL_COMP_SUM                            */
    int32_t  n_weight[CPOL_COMP_FIELDS];            /* 0: w = v; else 2 ... CPOL_COMP_MAX_TABLE breakpoints         */
    const float  *weight_v[CPOL_COMP_FIELDS];       /* [n_weight[k]] breakpoints in the field's linear units       */
    const double *weight_f[CPOL_COMP_FIELDS];       /* [n_weight[k]] values at the breakpoints                     */
    double   *sum[CPOL_COMP_FIELDS];                /* [n_blocks][n_z or absent][n_y][n_x]; a finishing call       */
    uint32_t *sum_skipped[CPOL_COMP_FIELDS];        /* likewise                                                    */
} cpol_composite_sums;

/* Neighbourhood verification: the sums of the fractions skill score (FSS; Roberts and Lean 2008) of ONE finished plane of a
 * composite against an observed map on the same grid, per block, threshold and neighbourhood size, reduced on the device, for
 * the user who verifies MAPS against observations.  Replaces in the reference: nothing (its users pull every map to the host and
 * run box filters there).  Pointed to by cpol_outputs.fractions; honoured only beside cpol_outputs.composite in a call that
 * FINISHES the composite's pass (phase & 2).  cosmo_pol_amd/neighbourhood.py states the same rule in NumPy (`sums`).
 * INPUT: the plane `plane` (an index into the fixed plane order of cpol_composite: max, height_of_max, lowest, height_of_lowest,
 * echo_top_0 ..., planes not requested absent) of field `field`, float32 m[n_blocks][n_y][n_x] exactly as k_comp_finish leaves
 * it where it lies on the device, empty cells NaN; `observed`, float32 o[n_y][n_x] on the same grid in the field's own linear
 * units, NaN = no echo or no data; `domain`, uint8 [n_y][n_x], non-zero = the cell belongs to the verification domain (NULL:
 * every cell does).
 * THRESHOLDS: 1 ... 4, each rounded once to float32, not NaN; -inf and +inf are allowed.
 * RADII: 1 ... 8 integers r, strictly ascending, 0 <= r <= 1023; the window is (2r + 1) x (2r + 1) cells.
 * BINARY MAPS, float32 comparisons alone: F[b][t] = domain && m == m && m >= thr[t]; O[t] = domain && o == o && o >= thr[t].
 * WINDOW COUNTS: NF[b][t][w][y][x] = the number of set cells (y', x') of F[b][t] with |y' - y| <= r_w and |x' - x| <= r_w INSIDE
 * the grid (the window is clipped at the border: nothing is set outside the grid); NO[t][w] likewise of O[t].
 * SUMS over the cells of the domain, uint64: diff2 = sum (NF - NO)^2, forecast2 = sum NF^2, observed2 = sum NO^2 per (b, t, w);
 * n_forecast = sum F, n_observed = sum O, n_domain = sum domain per (b, t).  FSS = 1 - diff2 / (forecast2 + observed2) is the
 * caller's division (neighbourhood.fss).
 * NO OVERFLOW (a condition, not a measurement): the grid has at most 1023 x 1023 < 2^20 cells (cpol_composite: at most 1024
 * edges per axis), so a window count is <= 1023^2 < 2^20 and fits the uint32 summed-area tables; its square and the square of a
 * difference are < 2^40; a sum over at most 2^20 cells is < 2^60 < 2^64.
 * Every intermediate is an integer: the result depends neither on the order of the additions nor on how the work is cut.
 * OUTPUTS: sums uint64 [n_blocks][n_thresholds][n_radii][3] (diff2, forecast2, observed2); totals uint64
 * [n_blocks][n_thresholds][3] (n_forecast, n_observed, n_domain).  n_blocks is the composite's.  `sums` and `totals` follow
 * p->outputs_on_device like the composite's `count`; `observed` and `domain` lie where cpol_member_verify.obs lies: host arrays
 * with outputs_on_device 0 (copied to the device first), else memory the device reads in place.
 * LIMITS (conditions, not measurements): the summed-area tables of all blocks and thresholds and of the observation,
 * (n_blocks + 1) * n_thresholds * (n_y + 1) * (n_x + 1) * 4 bytes, at most 1 GiB; fewer than 2^31 workgroups per launch.
 * CPOL_ERR_ARG, nothing queued, an open pass untouched, the context usable: fractions without composite; a composite call that
 * does not finish; a field that is not in composite->fields; a plane index outside the field's planes; n_thresholds outside
 * 1..4; a NaN threshold; n_radii outside 1..8; a radius < 0 or > 1023; radii not strictly ascending; NULL observed, sums or
 * totals; a limit exceeded.
 * Three kernels (k_frac_rows, k_frac_cols, k_frac_score, cpol_frac.inl) run behind k_comp_finish and before the output copy; a
 * call without the struct queues exactly what it queued before.  The wrapper cpol_fractions_ensemble, below the object cells, reduces the
 * blocks of the same call to neighbourhood ensemble probabilities on the same tables. */
#define CPOL_FRAC_MAX_THRESHOLDS 4
#define CPOL_FRAC_MAX_RADII 8
#define CPOL_FRAC_MAX_RADIUS 1023

/* Object cells: the connected components of the binary maps of a cpol_fractions, numbered, with ten integer attributes each, for
 * the user who verifies OBJECTS (SAL, MODE, CRA and every cell tracker start here).  Replaces in the reference: nothing (its users
 * pull every map to the host and label it there).  Pointed to by cpol_fractions.objects: the cells ride on a scored finishing call
 * (a caller who wants cells alone asks for one radius, 0).  cosmo_pol_amd/objects.py states the same rule in NumPy (`cells`).
 * INPUT: the binary maps of cpol_fractions, unchanged: domain && m == m && m >= thr, float32 comparisons, thresholds rounded once.
 * SOURCES: one map per source s and threshold t; sources 0 ... n_blocks - 1 are the blocks of the scored plane, source n_blocks is
 * the observed map, labelled once per call.
 * OBJECT: a maximal set of set cells connected through `connectivity` neighbours: 4 (edges) or 8 (edges and corners).
 * FIRST CELL: the cell of an object with the smallest flat index iy * n_x + ix.
 * FILTER: objects with fewer than `min_area` cells are dropped.
 * NUMBERING: the kept objects are numbered 1 ... n in ascending order of their first cell (with min_area = 1 the numbering of
 * scipy.ndimage.label).
 * ATTRIBUTES, CPOL_OBJ_WORDS = 10 uint32 words per kept object, in this order: first (the flat index of the first cell); area;
 * sum of ix; sum of iy; the inclusive bounding box x0, x1, y0, y1; peak_cell (the flat index of the peak); the float32 bits of
 * the peak value.  The PEAK is the largest value m (o for the observed map) of the object's cells in the TOTAL order of the
 * float32 values, in which -0.0 lies before +0.0 (the order of the ensemble quantiles): among -0.0 and +0.0 the peak is +0.0
 * wherever it lies; among cells of equal bits the one with the smallest flat index.  (NaN cells are never set.)
 * NO OVERFLOW (a condition, not a measurement): at most 1023 x 1023 cells, so an area is < 2^20, a sum of ix or iy is
 * < 2^20 * 2^10 = 2^30, every index < 2^20: all fit uint32.  Every attribute is a count, an integer sum, an integer extreme or a
 * comparison: the result does not depend on the order in which the hardware works.  Float sums over an object's cells (rain
 * volume, weighted centroids) are EXACT SUMS, below: they do not depend on that order either.
 * OUTPUTS: n_objects uint32 [n_blocks + 1][n_thresholds]: the TRUE number of kept objects, also beyond max_objects; table uint32
 * [n_blocks + 1][n_thresholds][max_objects][CPOL_OBJ_WORDS], 8-byte aligned: row k - 1 belongs to object k, rows at or beyond
 * n_objects are zero, objects beyond max_objects have no row; labels int32 [n_blocks + 1][n_thresholds][n_y][n_x] or NULL: the
 * object's number, 0 for background and dropped objects, complete even when the table overflows.  The three follow
 * p->outputs_on_device like `sums`.
 * LIMITS: the labelling scratch, (n_blocks + 1) * n_thresholds * (2 * n_y * n_x + n_y) * 4 bytes, at most 1 GiB.
 * CPOL_ERR_ARG, nothing queued, an open pass untouched, the context usable: connectivity other than 4 or 8; min_area < 1;
 * max_objects outside 1 ... 65535; NULL n_objects or table; a table that is not 8-byte aligned; the limit exceeded.
 * Kernels (k_obj_*, cpol_obj.inl) run behind k_frac_score: a label-equivalence union-find (L[i] <= i always, a union is an
 * atomic minimum).  No kernel waits on another workgroup; every loop carries a strictly decreasing unsigned integer.
 *
 * EXACT SUMS (`sums` = 1; the tail of the struct, a zero tail means off and a call without it queues exactly what it queued
 * before): the rain volume and the weighted first moments of every object and of the whole field, for SAL (Wernli et al. 2008)
 * and every weighted centroid.  cosmo_pol_amd/objects.py states the same rule (`exact_sum`, `weight_of`, `cells`).
 * SUMMAND: for a cell with plane value m (o for the observed map) the summand is w = m.  With a weight table (weight_v float32
 * strictly ascending, weight_f float64, n_weight breakpoints) it is w = float32(f(m)), f the piecewise-linear function that the
 * column of the height layers evaluates (composite.column_of), statement by statement: j = #{ weight_v <= m } - 1 (searchsorted
 * 'right' - 1, float32 comparisons); t = (m - v_j) / (v_j+1 - v_j), d = f_j+1 - f_j, p = t * d, f_j + p, each ONE float64
 * operation; 0 below the table, weight_f[n - 1] at and above its end; then ONE rounding to float32.  weight_f must be finite and
 * non-decreasing, so that the peak of w over an object is w(peak).
 * SKIPPED CELLS: a cell whose w is +-inf is not summed; it is counted in `skipped`.  NaN cells are never set.
 * PER KEPT OBJECT WITH A TABLE ROW: volume = sum w, moment_x = sum w * ix, moment_y = sum w * iy over its cells, each sum formed
 * EXACTLY and rounded ONCE to float64, round-to-nearest-even; an exact zero is +0.0; `skipped` uint32.  A float32 is an integer
 * multiple of 2^-149 and a product w * ix is exact (24 + 10 bits), so every sum is a sum of integers: it does not depend on the
 * order of the additions, and the float64 is math.fsum of the summands.
 * PER SOURCE, independent of the thresholds: the same three sums over every cell with domain && m == m (the whole field: SAL's
 * amplitude and first location term), and field_cells uint32 [2] = the cells summed, the cells skipped.
 * ACCUMULATORS (conditions, not measurements; cpol_obj.h): with the bits of w as +-M * 2^(E - 150), E = max(e, 1), M < 2^24,
 * sixteen signed 64-bit bins of the volume (bin E >> 4 takes +-M << (E & 15) < 2^39; fewer than 2^20 cells: |bin| < 2^59) and
 * thirty-two of each moment (bin E >> 3 takes +-(M * ix) << (E & 7); the sum of ix is < 2^30 by NO OVERFLOW above: |bin| <
 * 2^61), added with integer atomics, then propagated into one 384-bit integer and rounded by hand: the top 53 bits, the guard bit
 * and the sticky rest.
 * OUTPUTS: volume float64 [n_blocks + 1][n_thresholds][max_objects][3] (volume, moment_x, moment_y), 8-byte aligned, rows at or
 * beyond n_objects zero; skipped uint32 [n_blocks + 1][n_thresholds][max_objects]; field float64 [n_blocks + 1][3], 8-byte
 * aligned; field_cells uint32 [n_blocks + 1][2].  The four follow p->outputs_on_device like `table`.
 * LIMITS: the labelling scratch plus the accumulators, (16 + 32 + 32) * 8 bytes per table row and per source, plus the weight
 * table, at most 1 GiB.
 * CPOL_ERR_ARG as above: sums other than 0 or 1; a NULL output with sums on; volume or field not 8-byte aligned; n_weight
 * other than 0 or 2 ... 1024; NULL weight_v or weight_f; a breakpoint or value that is NaN or infinite; breakpoints not strictly
 * ascending; values that decrease; the limit exceeded.
 * Two kernels behind k_obj_decode: k_obj_sums (a wavefront per source and row; equal (object, bin) keys are combined inside the
 * wavefront before ONE atomic) and k_obj_sums_finish (a thread per sum: the rounding).
 *
 * MATCH (cpol_objects_match, below: a cpol_objects whose pad_ holds max_pieces, embedded as the first member; a zero pad_ means
 * off and a call without it queues exactly what it queued before): which forecast object lies on which observed object and by how
 * many cells, for object hits, misses and false alarms, MODE-style pairs and CRA displacement.  It needs neither `labels` nor the
 * exact sums; both may be on beside it and neither changes.  cosmo_pol_amd/objects.py states the same rule (`pieces_of_map`).
 * For every block b (0 ... n_blocks - 1) and threshold t:
 * LABEL MAPS: lf is the label map of source b, lo that of the observed map (source n_blocks), both at threshold t exactly as
 * `labels` defines them: kept objects only (min_area applied), numbers 1 ... n_objects, complete even beyond max_objects.
 * OVERLAP MAP: I = (lf > 0) & (lo > 0).
 * PIECE: a maximal set of cells of I connected through `connectivity`.  Every piece lies in exactly one forecast object and one
 * observed object.
 * NUMBERING: the pieces are numbered 1 ... n in ascending order of their first cell (the smallest flat index); no area filter.
 * PIECE ROW, CPOL_OBJ_WORDS uint32 words: first, area, sum of ix, sum of iy, x0, x1, y0, y1 (the object row's first eight words),
 * then forecast (the piece's number in lf) and observed (its number in lo).  NO OVERFLOW holds as above.
 * OUTPUTS: n_pieces uint32 [n_blocks][n_thresholds]: the TRUE count, also beyond max_pieces; pieces uint32 [n_blocks]
 * [n_thresholds][max_pieces][CPOL_OBJ_WORDS], rows at or beyond n_pieces zero; covered uint32 [n_blocks][n_thresholds][2]
 * [max_objects]: side 0, entry k - 1: the cells of forecast object k of block b that lie in I; side 1, entry k - 1: the cells of
 * observed object k that lie in I against block b; entries at or beyond min(n_objects, max_objects) of that side are zero.
 * `covered` is counted from the cells, so it is complete whatever max_pieces is.  The three follow p->outputs_on_device like
 * `table`.  Every number is a count, an integer sum, an integer extreme or a comparison: the result is exact in any order.
 * INVARIANTS (nothing overflowing): sum of pieces.area == sum of covered[0] == sum of covered[1] == the cells of I; covered[0]
 * [k - 1] <= the area of object k.
 * LIMITS: the piece scratch, n_blocks * n_thresholds * (2 * n_y * n_x + n_y) * 4 bytes, lies behind the labelling scratch and the
 * sums' accumulators; the total is at most 1 GiB.
 * CPOL_ERR_ARG as above: pad_ outside 0 ... 65535; NULL n_pieces, pieces or covered with match on; the limit exceeded; too many
 * workgroups.
 * Kernels behind everything above: k_match_runs (the overlap flag from the two (root, number) lookups, the piece runs, `covered`
 * with one integer atomic per run segment and side), then k_obj_merge, k_obj_flatten, k_obj_area, k_obj_count and k_obj_number on
 * the piece arrays, k_match_attr and k_match_decode.
 *
 * TRACK (cpol_objects_track, below: a cpol_objects_match embedded as the first member, announced by CPOL_OBJ_TRACK, bit 30 of
 * o.pad_; the low 16 bits of pad_ stay max_pieces of the match against the observed map, 0 meaning that match is off; a call
 * without the bit queues exactly what it queued before): the objects of one block followed into the next one, for storm tracks,
 * cell lifetimes, splits and merges and the motion field of a nowcast, when the blocks of the call are scan times.  It needs
 * neither `labels`, the exact sums nor the match; all may be on beside it and none changes.  cosmo_pol_amd/objects.py states the
 * same rule (`correlation_of_pair`, `shift_of`, `shift_labels`, `track_of_maps`).
 * A call has B = n_blocks >= 2 blocks and P = B - 1 pairs; pair p is (earlier = block p, later = block p + 1).  Per pair and
 * threshold t, le and ll are the label maps of the two blocks exactly as `labels` defines them, Ke = le > 0, Kl = ll > 0.
 * CORRELATION: for |dy|, |dx| <= S = max_shift (0 ... CPOL_TRACK_MAX_SHIFT): C[dy + S][dx + S] = #{(y, x): Ke[y][x] and
 * Kl[y + dy][x + dx]}, both cells inside the grid; uint32 (a count is below 2^20).  S may exceed the grid's sides: such offsets
 * count 0.
 * SHIFT: the (dy, dx) with the largest C; ties go to the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx.  An
 * all-zero table gives (0, 0).
 * GIVEN SHIFTS: max_shift = -1 and shifts_in int32 [P][n_thresholds][2] (dy, dx), a HOST array whatever outputs_on_device says,
 * |dy|, |dx| <= CPOL_TRACK_MAX_GIVEN (1023), read and checked before anything is queued and copied into `shift`; no correlation
 * is then computed and `correlation` is not touched.
 * SHIFTED OVERLAP: le'[y][x] = le[y - dy][x - dx] inside the grid, 0 outside.  The pieces, n_pieces and covered of the pair are
 * those of MATCH with lf = le' and lo = ll, in the later block's frame: `forecast` is the object's number in the earlier block,
 * `observed` its number in the later block; covered side 0 counts cells of the earlier objects, side 1 cells of the later ones.
 * The INVARIANTS of MATCH hold.
 * OUTPUTS: correlation uint32 [P][n_thresholds][2S + 1][2S + 1] or NULL = not wanted (the counters then lie in the scratch);
 * shift int32 [P][n_thresholds][2]; n_pieces uint32 [P][n_thresholds]: the TRUE count; pieces uint32 [P][n_thresholds]
 * [max_pieces][CPOL_OBJ_WORDS], rows at or beyond n_pieces zero; covered uint32 [P][n_thresholds][2][max_objects].  All follow
 * p->outputs_on_device like `table`.  Every number is an integer: the result is exact in any order.
 * LIMITS: the track scratch lies behind everything above on an 8-byte boundary: the packed masks uint64 [n_blocks][n_thresholds]
 * [n_y][ceil(n_x / 64)], then P * n_thresholds piece maps of (2 * n_y * n_x + n_y) * 4 bytes, then, with max_shift >= 0 and a
 * NULL `correlation`, the counters; the total is at most 1 GiB.
 * CPOL_ERR_ARG as above, with nothing queued: n_blocks < 2; max_shift outside -1 ... 32; max_shift == -1 without shifts_in, or
 * shifts_in with max_shift >= 0; a given shift beyond +-1023; max_pieces outside 1 ... 65535; NULL shift, n_pieces, pieces or
 * covered; the limit exceeded; too many workgroups.  pad_ negative or with any of bits 16 ... 29 set is refused as before.
 * Kernels behind everything above: k_track_bits (Ke of every block and threshold packed with a ballot per 64 cells),
 * k_track_corr (popcounts of earlier words against funnel-shifted later words; one integer atomic per counter and workgroup),
 * k_track_shift (a wavefront per pair and threshold: the argmax under the tie order), k_track_runs (k_match_runs with the earlier
 * block's lookup at cell - shift, the shift read from device memory), then k_obj_merge, k_obj_flatten, k_obj_area, k_obj_count
 * and k_obj_number on the track's piece arrays, k_track_attr and k_match_decode.
 * NOT BUILT: tracking across calls; tracks of layered composites; per-object (local) shifts; a process group. */
#define CPOL_OBJ_WORDS 10
#define CPOL_OBJ_MAX_OBJECTS 65535
#define CPOL_OBJ_TRACK (1 << 30)    /* in cpol_objects.pad_: the struct is the first member of a cpol_objects_track */
#define CPOL_TRACK_MAX_SHIFT 32
#define CPOL_TRACK_MAX_GIVEN 1023
typedef struct cpol_objects {
    int32_t  connectivity;      /* 4 or 8                                                                          */
    int32_t  min_area;          /* >= 1                                                                            */
    int32_t  max_objects;       /* 1 ... 65535 table rows per (source, threshold)                                  */
    int32_t  pad_;              /* 0, or max_pieces (1 ... 65535) when this struct is the first member of a cpol_objects_match; CPOL_OBJ_TRACK */
    uint32_t *n_objects;        /* [n_blocks + 1][n_thresholds]                                                    */
    uint32_t *table;            /* [n_blocks + 1][n_thresholds][max_objects][CPOL_OBJ_WORDS]                       */
    int32_t  *labels;           /* [n_blocks + 1][n_thresholds][n_y][n_x] or NULL = not wanted                     */
    /* the exact sums: a zero-initialised tail means off */
    int32_t  sums;              /* 0 or 1                                                                          */
    int32_t  n_weight;          /* 0: w = m; else 2 ... CPOL_COMP_MAX_TABLE breakpoints of the weight table        */
    const float  *weight_v;     /* [n_weight] breakpoints in the plane's units, strictly ascending                 */
    const double *weight_f;     /* [n_weight] values at the breakpoints, finite and non-decreasing                 */
    double   *volume;           /* [n_blocks + 1][n_thresholds][max_objects][3]: volume, moment_x, moment_y         */
    uint32_t *skipped;          /* [n_blocks + 1][n_thresholds][max_objects]                                       */
    double   *field;            /* [n_blocks + 1][3]: the same sums over the whole field of every source           */
    uint32_t *field_cells;      /* [n_blocks + 1][2]: cells summed, cells skipped                                   */
} cpol_objects;

/* MATCH (above): cpol_fractions.objects points at `o`; the library reads beyond it only when o.pad_ != 0 */
typedef struct cpol_objects_match {
    cpol_objects o;             /* o.pad_ = max_pieces, 1 ... 65535 piece rows per (block, threshold)                 */
    uint32_t *n_pieces;         /* [n_blocks][n_thresholds]                                                          */
    uint32_t *pieces;           /* [n_blocks][n_thresholds][max_pieces][CPOL_OBJ_WORDS]                              */
    uint32_t *covered;          /* [n_blocks][n_thresholds][2][max_objects]: forecast side, observed side             */
} cpol_objects_match;

/* TRACK (above): cpol_fractions.objects points at `m.o`; the library reads beyond `m` only when m.o.pad_ has CPOL_OBJ_TRACK.
 * The low 16 bits of m.o.pad_: max_pieces of the match against the observed map, 0 = that match is off (m's pointers unread). */
typedef struct cpol_objects_track {
    cpol_objects_match m;
    int32_t  max_shift;         /* 0 ... CPOL_TRACK_MAX_SHIFT: the correlation's reach; -1: the shifts are given              */
    int32_t  max_pieces;        /* 1 ... 65535 piece rows per (pair, threshold)                                              */
    const int32_t *shifts_in;   /* host [n_blocks - 1][n_thresholds][2] (dy, dx) with max_shift == -1, else NULL              */
    uint32_t *correlation;      /* [n_blocks - 1][n_thresholds][2 max_shift + 1][2 max_shift + 1] or NULL = not wanted        */
    int32_t  *shift;            /* [n_blocks - 1][n_thresholds][2]: dy, dx                                                   */
    uint32_t *n_pieces;         /* [n_blocks - 1][n_thresholds]                                                              */
    uint32_t *pieces;           /* [n_blocks - 1][n_thresholds][max_pieces][CPOL_OBJ_WORDS]                                  */
    uint32_t *covered;          /* [n_blocks - 1][n_thresholds][2][max_objects]: earlier side, later side                     */
} cpol_objects_track;

/* Neighbourhood ensemble probabilities: what a convective-scale ensemble publishes of its members' maps -- the neighbourhood
 * ensemble probability (NEP) and the neighbourhood maximum ensemble probability (NMEP; Schwartz and Sobash 2017, Mon. Wea. Rev.
 * 145, 3397-3418), the ensemble FSS of the ensemble-mean fraction (Schwartz et al. 2010; Duc et al. 2013) and a reliability
 * table, from which the Brier score, the reliability diagram and the ROC follow.  Replaces in the reference: nothing (its users
 * pull every member's map to the host and box-filter it there).  Pointed to by cpol_fractions_ensemble.probabilities (below: a
 * cpol_fractions with CPOL_FRAC_ENSEMBLE in its n_radii, embedded as the first member, the way cpol_objects_match embeds a
 * cpol_objects; cpol_fractions itself keeps its size and its last member): the product rides on a scored finishing call and
 * reads the summed-area tables that call has built.  cosmo_pol_amd/neighbourhood.py states the same
 * rule in NumPy (`ensemble_sums`).
 * THE RULE
 * Inputs are those of cpol_fractions, unchanged.  F[b][t], O[t], NF[b][t][w][y][x] and NO[t][w][y][x] are the binary maps and
 * clipped window counts defined there.  M = n_blocks; in an ensemble call a block is a member.
 * Per threshold t, radius index w and cell:
 *   S[t][w][y][x] = sum over b of NF[b][t][w][y][x] (uint32).  NEP is S / (M * window_cells); the division is the host's.
 *   A[t][w][y][x] = #{ b : NF[b][t][w][y][x] > 0 } (uint32, 0 ... M).  NMEP is A / M.
 *   OA[t][w][y][x] = NO[t][w][y][x] > 0.
 * Both maps are written for EVERY cell of the grid.  The domain only decides which cells are set and which cells are summed.
 * Sums over the cells of the domain, uint64:
 *   prob_sums[t][w][3] = (diff2, forecast2, observed2): diff2 = sum (S - M * NO)^2, forecast2 = sum S^2, observed2 = M^2 * sum
 *   NO^2.  neighbourhood.fss applied to these three gives the ensemble FSS unchanged.  With M == 1 they equal block 0's row of
 *   `sums`.
 *   reliability[t][w][k][o], k = 0 ... M, o = 0 | 1: the number of domain cells with A == k and OA == o.  At radius 0 this is the
 *   classic table "k of M members exceed, observed yes or no".  At larger radii it is the NMEP against the neighbourhood-maximum
 *   observation.  Every [t][w] slice sums to n_domain.
 * Limits are conditions, not measurements.
 *   1 <= n_blocks <= CPOL_FRAC_PROB_MAX_BLOCKS (256); it bounds `reliability` and the kernel's LDS table.
 *   NO OVERFLOW, checked before anything is queued.  Let c = min(2 * r_max + 1, n_y) * min(2 * r_max + 1, n_x).  The call is
 *   refused unless M * c < 2^32 and n_y * n_x * (M * c)^2 < 2^64.  |S - M * NO| <= M * c, so the bound covers all three sums.
 *   (It passes for 300 x 300 cells, 21 members, any radius; for 1023^2, 128 members, radius 20; for 1023^2, 256 members, radius
 *   32.  It refuses 1023^2, 128 members, radius 1023.)
 * The result depends neither on the order of the blocks nor on how the work is cut.
 * OUTPUTS: prob_sums uint64 [n_thresholds][n_radii][3]; reliability uint64 [n_thresholds][n_radii][n_blocks + 1][2]; member_sum
 * and member_any (the S and the A maps) uint32 [n_thresholds][n_radii][n_y][n_x], each or NULL = not wanted.  They follow
 * p->outputs_on_device like `sums`.  The struct may stand beside `objects`: the two are independent readers of the same tables.
 * CPOL_ERR_ARG, nothing queued, an open pass untouched, the context usable: NULL prob_sums or reliability; n_blocks > 256; the
 * overflow condition.
 * One kernel (k_frac_members, cpol_frac_prob.inl) runs directly behind k_frac_score and before the object kernels; it reads only
 * the summed-area tables and the domain.  A call without the struct queues exactly what it queued before. */
#define CPOL_FRAC_PROB_MAX_BLOCKS 256
typedef struct cpol_fraction_probabilities {
    uint64_t *prob_sums;        /* [n_thresholds][n_radii][3]                                                      */
    uint64_t *reliability;      /* [n_thresholds][n_radii][n_blocks + 1][2]                                        */
    uint32_t *member_sum;       /* [n_thresholds][n_radii][n_y][n_x] or NULL = not wanted: the S maps              */
    uint32_t *member_any;       /* [n_thresholds][n_radii][n_y][n_x] or NULL = not wanted: the A maps              */
} cpol_fraction_probabilities;

typedef struct cpol_fractions {
    int32_t  field;           /* the field whose plane is scored: one of composite->fields                        */
    int32_t  plane;             /* index into that field's plane order                                             */
    int32_t  n_thresholds;      /* 1 ... 4                                                                         */
    int32_t  n_radii;           /* 1 ... 8                                                                         */
    double   thresholds[CPOL_FRAC_MAX_THRESHOLDS];      /* the field's own linear units, rounded once to float32   */
    int32_t  radii[CPOL_FRAC_MAX_RADII];                /* strictly ascending, 0 ... 1023                          */
    const float   *observed;    /* [n_y][n_x]                                                                      */
    const uint8_t *domain;      /* [n_y][n_x] or NULL = every cell                                                 */
    uint64_t *sums;             /* [n_blocks][n_thresholds][n_radii][3]                                            */
    uint64_t *totals;           /* [n_blocks][n_thresholds][3]                                                     */
    cpol_objects *objects;      /* NULL (a zero-initialised struct): off.  The object cells of the same binary maps */
} cpol_fractions;

/* NEIGHBOURHOOD ENSEMBLE PROBABILITIES (cpol_fraction_probabilities, above): cpol_outputs.fractions points at `f`; the library
 * reads beyond it only when f.n_radii > 0 carries CPOL_FRAC_ENSEMBLE (n_radii = 1 ... 8, or-ed with the flag; a zero-initialised
 * cpol_fractions has no flag: off).  With the flag and probabilities == NULL the product is off too. */
#define CPOL_FRAC_ENSEMBLE 0x10000
typedef struct cpol_fractions_ensemble {
    cpol_fractions f;           /* f.n_radii = the number of radii | CPOL_FRAC_ENSEMBLE                               */
    cpol_fraction_probabilities *probabilities;     /* NEP, NMEP, the ensemble FSS's sums and the reliability table of
                                   the blocks of the same call; NULL: off                                             */
} cpol_fractions_ensemble;

/* Terrain shadowing (cpol_sweep_params.terrain_shadow, cpol_outputs.visibility; cosmo_pol_amd/shadow.py states the same rule in
 * NumPy).  Replaces in the reference: nothing that runs -- interpolation_c.c:92-102 writes NaN into every gate from the first one
 * below the topography onward ("We hit a mountain") and its own loop overwrites those gates again, so that every gate depends on
 * itself alone.  That accident stays the default (terrain_shadow = 0).
 *
 * A ROW is one sub-beam of one ray.  Its codes c[g], g = 0 .. n_gates-1, are as the interpolation leaves them: 0 valid, +1 above
 * the model top, -1 below the topography or variable 0 NaN (2: outside the domain).
 *   first = min{ g : c[g] == -1 }, or n_gates when there is none.
 *   For every g >= first: c[g] = -1 and every staged model variable of that sub-beam gate becomes NaN (a +1 behind the hit becomes
 *   -1; the NaN is the one the interpolation writes for a gate below the topography).
 *   Gates g < first keep their bits.  The geometry arrays (lats, lons, dist, heights, elev) are never touched.
 *   The step runs after the interpolation (in any interpolating form) and before melting, the 'ml' weights, the classification and
 *   everything behind them: the rest of the launch sequence sees a shadowed gate exactly as it sees a gate below the topography.
 * With terrain_shadow = 1 the sweep takes the unfused launch forms (k_interp_sweep / record / replay or the member forms, then
 * k_terrain_shadow, then the second half): no k_interp_classify, no presence words, no graph replay.  cpol_interp_subbeams exports
 * the shadowed columns.  In an ensemble call every member's rows are shadowed from that member's own codes.
 *
 * VISIBILITY, per ray and gate, float64: S = +0.0; for s ascending S += sub_w[s] where the (shadowed, if shadowing is on) code
 * c[ray, s, gate] != -1; visibility = S / W with W the sum of sub_w[s] ascending from +0.0.  Exactly 1.0 where no sub-beam is
 * blocked, exactly 0.0 where all are; without shadowing it reports the local below-topography sub-beams alone.  cpol_run_columns
 * computes it from the ingested masks.
 *
 * CPOL_ERR_ARG, nothing queued, the context usable: terrain_shadow outside 0 / 1; terrain_shadow with spaceborne geometry (the
 * gates of a swath run from the satellite downward); terrain_shadow in cpol_run_columns (the caller's masks stand, and nobody
 * should believe they were shadowed); visibility with per-gate weights (integration scheme 'ml').
 * cpol_debug_read "terrain_shadow_rows" runs k_terrain_shadow alone on caller arrays (a test hook, see cpol_debug_read). */

/* Hydrometeor contributions: per gate and per hydrometeor slot the radar fields that the species ALONE gives, which species are
 * present, which one dominates ZH and by what share.  Replaces in the reference: nothing (it folds the per-species sums with
 * np.nansum(sz_integ, axis=1), doppler_scatter.py:400, and hands back the totals; its users re-run the sweep once per species).
 * Pointed to by cpol_outputs.species; honoured by cpol_run_sweep and by a time-blended cpol_run_sweep_members.
 * INPUT per gate: the rows sz_integ[gate][j][0 .. 11] of the call, float32, j = 0 .. n_hydro-1 in slot order -- the sub-beam sums
 * of species j as k_final / k_subbeam_sum form them, a row of NaNs where the species has no item at the gate -- and ZHf, the
 * call's own ZH of the gate as delivered, after the range scans and the sensitivity cut.  The constants are the launch
 * sequence's: c_zh = (float)p->c_zh, c_kdp = (float)(1e-3 * (180 / pi) * p->wavelength), c_2w = (float)(2 * p->wavelength).
 * RULE per gate and species j, t[c] = the row's column c; every operation ONE float32 operation (no contraction), in this order:
 *     t[c] == 0.0f (either sign) becomes NaN                                        (quirk Q5, as the totals apply it)
 *     two_pi = (float)(2 pi); b = t0 - t1 - t2 + t3; cc = t0 + t1 + t2 + t3         (left to right)
 *     ZH_j = c_zh * (two_pi * b);  ZV_j = c_zh * (two_pi * cc)
 *     ZDR_j = (two_pi * b) / (two_pi * cc)       the INTRINSIC ratio: the total's ZDR is attenuated, a species' ZDR is not
 *     KDP_j = c_kdp * (t10 - t8)
 *     ATT_H_j = 4.343e-3f * (c_2w * t11);  ATT_V_j = 4.343e-3f * (c_2w * t9)
 *     RHOHV_j = sqrtf(((t4 + t7) * (t4 + t7) + (t6 - t5) * (t6 - t5)) / (b * cc))
 *     DELTA_HV_j = (float)atan2((double)(t5 - t6), (double)(-t4 - t7))
 * CENSORING: where ZHf is NaN, ZH_j, ZV_j, ZDR_j, KDP_j and RHOHV_j become NaN for every j; ATT_H_j, ATT_V_j and DELTA_HV_j keep
 * their values (the set the sensitivity cut touches and leaves in the totals).
 * present: bit j set iff ZH_j == ZH_j after censoring.  dominant: starts at 255 with no best value; for j ascending, j is taken
 * when bit j of `present` is set and either nothing has been taken yet or ZH_j > best (strict: a tie keeps the lower slot).
 * share: S = the float32 sum of the ZH_j with bit j set, j ascending, from +0.0f; share = ZH_dominant / S; NaN where dominant is 255.
 * The per-species arrays are species-major, [n_hydro][n_rays * n_gates], as model_vars is variable-major.  sz: the rows
 * themselves.  An array left NULL is not written and costs no store.  The pointers follow p->outputs_on_device like every other
 * array (mode 2: they count for the one-copy window rule).
 * CPOL_ERR_ARG, nothing queued, the context usable: every pointer NULL; n_hydro different from the staged slots; any other
 * product in the same call; cpol_run_columns; cpol_run_sweep_members with time_blend == 0 (the ensemble form).
 * LAUNCH: a call with the struct takes the general launch sequence, as the debug reads do (the single-beam kernels keep an absent
 * species as 0.f in registers and never form the NaN-marked rows); every per-gate array has the bits of the plain call.  ONE
 * kernel (k_species, one lane per gate) runs behind the range scans and the cut and before the output copy.  Without the struct
 * a call launches what it always launched. */
typedef struct cpol_species {
    float   *ZH, *ZV, *ZDR, *KDP, *RHOHV, *DELTA_HV, *ATT_H, *ATT_V;  /* each [n_hydro][n_rays * n_gates], NULL = not wanted */
    uint8_t *dominant, *present;                                      /* [n_rays * n_gates] */
    float   *share;                                                   /* [n_rays * n_gates] */
    float   *sz;                                                      /* [n_rays * n_gates][n_hydro][12]: sz_integ itself */
    int32_t  n_hydro, pad_;                                           /* must equal the staged slots */
} cpol_species;

/* cpol_outputs.  A call takes AT MOST ONE product behind its arrays: superob, member_stats (member_verify rides on it),
 * spectrum_moments, histogram, composite (fractions, with its objects, rides on it) or species; any two are refused (CPOL_ERR_ARG). */
typedef struct {
    /* all [n_rays * n_gates]; NULL = not wanted */
    float  *ZH, *ZV, *ZDR, *KDP, *DELTA_HV, *PHIDP, *RHOHV, *ATT_H, *ATT_V;
    double *RVEL;
    double *mask;
    cpol_species *species;      /* NULL (a zero-initialised struct): off.  The radar fields per hydrometeor species, the dominant
                                   species and its share, see cpol_species.  (In front of the members that are pinned where
                                   they are.) */
    double *lats, *lons;        /* central sub-beam                             */
    float  *dist, *heights;
    double *visibility;         /* [n_rays*n_gates] float64, NULL = not wanted: the visible share of the antenna pattern per gate,
                                   see "Terrain shadowing" below.  Geometry rows only: in ensemble and timed calls it is stored
                                   once, like lats (an ensemble call reads the codes of its first member)                        */
    double *model_vars;         /* [n_vars][n_rays*n_gates] (integrate_model)   */
    cpol_fractions *fractions;  /* NULL (a zero-initialised struct): off.  The fractions skill score's sums of one finished
                                   plane of `composite` against an observed map, see cpol_fractions */
    float  *sz_total;           /* [n_rays*n_gates][12]  (debug / parity)       */
    cpol_composite *composite;  /* NULL (a zero-initialised struct): off.  Maps of the radar fields above (column maximum, lowest
                                   gate, echo tops), see cpol_composite */
    cpol_histogram *histogram;  /* NULL (a zero-initialised struct): off.  Counts of the radar fields above over many gates,
                                   see cpol_histogram */
    double *DSPECTRUM;          /* [n_rays*n_gates][n_vbins]  (Doppler scheme 3) */
    cpol_member_verify *member_verify;  /* NULL (a zero-initialised struct): off.  The members of the pass of member_stats scored
                                   against observations, see cpol_member_verify */
    int8_t *mask_sum8;          /* [n_rays*n_gates] the radial mask as what it is made of: the SUM over the sub-beams of
                                   their mask codes (-1 below the topography, 0, +1 above the model top, 2 outside the
                                   domain; doppler_scatter.py:472-477), one byte per gate instead of the eight of `mask`.
                                   mask = mask_sum8 / n_sub, then values in (-1, 0] -> 0: the caller's two NumPy statements.
                                   Needs 2 * n_sub <= 127.  When it is asked for and `mask` is not, `mask` is not written. */
    cpol_spectrum_moments *spectrum_moments;    /* NULL (a zero-initialised struct): off.  The moments of every gate's Doppler
                                   spectrum (Doppler scheme 3), see cpol_spectrum_moments */
    cpol_member_stats *member_stats;  /* NULL (a zero-initialised struct): off.  The call's member(s) folded into the
                                   context's running ensemble statistics, see cpol_member_stats */
    cpol_superob *superob;     /* NULL (a zero-initialised struct): off.  Window averages of the fields above, see cpol_superob.
                                   Stays the LAST member */
} cpol_outputs;

typedef struct {
    int64_t n_subbeam_gates;    /* N_sbg                                        */
    int64_t n_valid_items;      /* N_valid: (sub-beam gate, hydrometeor), QM>0  */
    int64_t n_gates;            /* output gates                                 */
    int64_t n_work_units;       /* work units of the integrating PSD kernels    */
    float   ms_traj, ms_interp, ms_classify, ms_bucket, ms_psd, ms_final, ms_total;
    int32_t n_table_items;      /* of n_valid_items: finished from the integral tables
                                   (the others were integrated bin by bin)      */
    int32_t pad_;
} cpol_counters_t;

CPOL_API int  cpol_create(int device, cpol_ctx **out);
CPOL_API void cpol_destroy(cpol_ctx *ctx);
/* A LANE of `parent`: a context that shares the parent's staged model cube and
 * scattering tables (read-only, no copy) and owns its own HIP stream, work buffers and
 * counters, so that independent sweeps (the elevations of a volume scan, consecutive
 * scans) are in flight together -- the reference runs them one after the other
 * (radar_operator.py:429-432).  Fork after staging; stage calls fail on a lane and on a
 * parent with live lanes; destroy lanes before their parent.  One host thread per lane. */
CPOL_API int  cpol_fork(cpol_ctx *parent, cpol_ctx **out);
CPOL_API const char *cpol_last_error(cpol_ctx *ctx);
/* use an externally created hipStream_t (e.g. torch's current stream); NULL = own stream */
CPOL_API int  cpol_set_stream(cpol_ctx *ctx, void *hip_stream);
/* waits for the context's stream.  Also the point where a DEFERRED domain error surfaces:
 * sweeps with outputs_on_device = 1 / 2 return before their kernels ran, so a gate outside
 * the model domain (reference: IndexError, interpolation.py:572-580) sets a sticky error word
 * on the device that stays set over later sweeps until cpol_synchronize or cpol_counters has
 * reported it ONCE as CPOL_ERR_DOMAIN (then it is cleared). */
CPOL_API int  cpol_synchronize(cpol_ctx *ctx);
/* page-locked host memory owned by the context (freed by cpol_host_free / cpol_destroy): the
 * target of outputs_on_device = 2, so that the device-to-host copy of one sweep overlaps the
 * kernels of the next (other lanes) instead of being staged through pageable memory.
 * ctx = NULL: a context-free block owned by the caller until cpol_host_free(NULL, p) -- for host-side
 * pools whose blocks (results handed to the user) must outlive the contexts that filled them; the
 * caller makes sure no copy into the block is in flight when it frees or re-uses it */
CPOL_API int  cpol_host_alloc(cpol_ctx *ctx, size_t bytes, void **out);
CPOL_API int  cpol_host_free(cpol_ctx *ctx, void *p);
/* a context-free block as cpol_host_alloc(NULL, ...) gives, taken from the NUMA node next to GPU
 * `device` whatever the calling thread's current device is (one process per GPU on a two-socket host:
 * helper threads have never called hipSetDevice); freed by cpol_host_free(NULL, p) */
CPOL_API int  cpol_host_alloc_near(int device, size_t bytes, void **out);
/* "0000:75:00.0" of GPU `device` (len >= 16): /sys/bus/pci/devices/<id>/numa_node and local_cpulist
 * tell a one-process-per-GPU launcher which cores to run the rank on (the reference's pool is not
 * placed at all, radar_operator.py:402) */
CPOL_API int  cpol_device_pci_bus_id(int device, char *buf, int len);
/* free and total device memory of the context's GPU in bytes (hipMemGetInfo; `free_bytes` also counts what the
 * context's own grow-only work buffers hold already: the room a launch sequence of THIS context has), and an estimate of
 * the work-buffer bytes ONE sub-beam gate of a launch sequence needs with the hydrometeors staged
 * now (`per_gate`: about 1.2 KB with six species): what a caller that packs many sweeps into one
 * cpol_run_sweep call sizes its batches by (the reference processes one radial at a time,
 * radar_operator.py:431).  Not counted in `per_gate`: the gate stencil store of the root context -- 69 bytes per gate of
 * every single-beam scan geometry seen twice, up to its budget (1 GiB unless cpol_debug_read "stencil_budget" says otherwise);
 * cpol_debug_read "stencil" reports the bytes it holds, and `free_bytes` sees them as used memory */
CPOL_API int  cpol_mem_info(cpol_ctx *ctx, size_t *free_bytes, size_t *total_bytes, size_t *per_gate);
/* the HIP stream (hipStream_t) the context launches on: to order foreign work (copies,
 * collectives) against a sweep with events */
CPOL_API int  cpol_get_stream(cpol_ctx *ctx, void **hip_stream);

/* data[v] and zlevels: [nz][ny][nx] float32, C order (x = rotated longitude
 * fastest), level 0 = model top; llc = (Lo1, La1), urc = (Lo2, La2), res =
 * (dlon, dlat) as float32; south_pole = (lat, lon) of the rotated south pole. */
CPOL_API int  cpol_stage_model(cpol_ctx *ctx, int n_vars, const float *const *data,
                      const float *zlevels, int nz, int ny, int nx,
                      const float llc[2], const float urc[2], const float res[2],
                      const double south_pole[2]);

/* ---- ensemble members: many model states under ONE set of scattering / integral tables ------------------------------------
 * Replaces in the reference: nothing -- the reference runs one model state per process.
 * The cube staged by cpol_stage_model / cpol_stage_model_packed is member 0.  cpol_stage_member stages the variables of
 * another state of the SAME model: same n_vars and variable order, same [nz][ny][nx] shape, same grid, same level heights
 * (they are staged once, with member 0, and shared).  member = cpol_num_members(ctx) appends, a smaller index restages that
 * member in place (0: the cube of cpol_stage_model, heights kept).  Device memory per member: exactly n_vars * nz * ny * nx * 4
 * bytes.  Staging a member does not touch the scattering tables or the integral tables (no rebuild).  Out of memory:
 * CPOL_ERR_NOMEM, the context stays usable with what was staged before.  cpol_stage_model and cpol_stage_model_packed drop all
 * members >= 1.  Like the cube, members belong to the root context and are shared by its lanes: stage before cpol_fork (the
 * call fails on a lane and on a context with live lanes). */
CPOL_API int  cpol_stage_member(cpol_ctx *ctx, int member, int n_vars, const float *const *data);
/* staged members including member 0 (0: no model staged); on a lane: its parent's */
CPOL_API int  cpol_num_members(cpol_ctx *ctx);
/* Every later cpol_run_sweep, cpol_interp_subbeams and cpol_interp_points of THIS context (a lane has its own selection; a new
 * lane starts with its parent's) reads the variables of `member`: a pointer swap, no copy.  A sweep after cpol_select_member(k)
 * carries the bits of a context staged with member k alone; a captured HIP graph is captured again.  CPOL_ERR_ARG: not staged. */
CPOL_API int  cpol_select_member(cpol_ctx *ctx, int member);

/* ---- model input in GRIB-1 simple packing, unpacked and derived on the device ------------------------------
 * One packed plane (one GRIB message): the bit string of BDS octet 12 onwards as it lies in the file (host memory),
 * and what turns its unsigned integers X into values (cosmo_pol_amd/grib1.py), in float64:
 *   t = R + ldexp(X, E);  D > 0: t / 10^D;  D < 0: t * 10^-D;  value = (float)t        (n_bits = 0: X = 0) */
typedef struct {
    const void *octets;         /* value i at bit i * n_bits, most significant bit first; NULL allowed with n_bits = 0 */
    int64_t  n_octets;          /* >= ceil(ny * nx * n_bits / 8)                                                   */
    double   ref_value;         /* R (the IBM single of BDS octets 7-10, converted exactly)                         */
    int32_t  bin_scale;         /* E                                                                                */
    int32_t  dec_scale;         /* D                                                                                */
    int32_t  n_bits;            /* 0 ... 32                                                                         */
    int32_t  flip_rows;         /* 1: rows stored north to south (scanning mode 0x00): flipped on unpacking          */
    int32_t  field;             /* raw-field index (stage_model_packed) | unused (unpack_planes: plane i -> out[i])  */
    int32_t  level;             /* 0-based level of the raw field (0 = model top)                                   */
} cpol_packed_plane;

#define CPOL_MAX_RAW_FIELDS 32
#define CPOL_MAX_LOAD       8
/* how a staged variable comes out of the raw fields (model_io.derive / read_model_file, operand by operand in float64) */
#define CPOL_RECIPE_COPY       0    /* the raw field `source` as it is (U, V, T; W or EDR on nz levels)              */
#define CPOL_RECIPE_HALF_MEAN  1    /* float32(0.5 * (x[k] + x[k + 1])) of a raw field on nz + 1 levels (W, EDR)     */
#define CPOL_RECIPE_RHO        2    /* air density P / (r_d T (1 + rv_rd_m1 QV - load))                              */
#define CPOL_RECIPE_TIMES_RHO  3    /* raw field `source` x the unrounded air density (Q*_v, QN*_v)                  */
#define CPOL_RECIPE_ZEROS      4    /* 0 (QNI_v of a file without QNI)                                              */
typedef struct {
    int32_t nz, ny, nx;                             /* full levels, rows, columns                                   */
    int32_t n_fields;                               /* raw fields the planes belong to                              */
    int32_t field_levels[CPOL_MAX_RAW_FIELDS];      /* levels of each raw field: nz, or nz + 1 (half levels)         */
    int32_t field_p, field_t, field_qv, field_hhl;  /* raw-field indices; HHL on nz + 1 levels (means) or nz (copy)  */
    int32_t n_load;                                 /* condensate fields subtracted in the density, in the order     */
    int32_t field_load[CPOL_MAX_LOAD];              /* they are summed (QC, QR, QS, QG, QI: those present)           */
    int32_t n_vars;                                 /* staged variables, in the order of the hydrometeor descriptors */
    int32_t recipe[CPOL_MAX_VARS];                  /* CPOL_RECIPE_*                                                */
    int32_t source[CPOL_MAX_VARS];                  /* raw-field index of COPY / HALF_MEAN / TIMES_RHO               */
    double  r_d, rv_rd_m1;                          /* R_d and R_v / R_d - 1 as the host folds them                  */
    float   llc[2], urc[2], res[2];                 /* as for cpol_stage_model                                       */
    double  south_pole[2];
} cpol_packed_model;

/* The staging of cpol_stage_model from packed planes: the octets travel to the device as they are, k_grib_unpack
 * turns them into float32 planes in a scratch cube (freed before the call returns), k_model_derive writes the
 * staged variables, the level heights and the (top, lowest) pairs.  Every (field, level) of `m` must come exactly
 * once.  The staged cube carries the bits model_io.read_model_file + cpol_stage_model give for the same file.
 * CPOL_ERR_ARG leaves the context and its staged model as they were. */
CPOL_API int  cpol_stage_model_packed(cpol_ctx *ctx, const cpol_packed_model *m, const cpol_packed_plane *planes,
                             int n_planes);
/* k_grib_unpack alone: n_planes planes of ny x nx values -> out [n_planes][ny][nx] float32 (host memory), rows
 * south to north.  Needs no staged model or tables. */
CPOL_API int  cpol_unpack_planes(cpol_ctx *ctx, const cpol_packed_plane *planes, int n_planes, int ny, int nx,
                        float *out);

/* table: float64 [n_e][n_t][n_d][12]; pre: [n_d] (or NULL) host-evaluated
 * N0*D^mu | D^mu; dnu: [n_d] D^nu; aux: family-specific per-bin tables.
 * Melting family with tab_degree = CPOL_MELT_DEGREE: aux = [n_t][2] (centre and 1 / half-width
 * of the wet-fraction interval of every bin of the second axis) followed by
 * [n_t][n_d][CPOL_MELT_FUNCS][CPOL_MELT_DEGREE + 1] monomial coefficients in
 * u = (fw - centre) / half-width of
 *   D_r(fw, k)   melted-equivalent diameter of bin k      (hydrometeors.py:382-383)
 *   G(fw, k)     N_r0 sqrt(D_r) V_r / V  dD_r/dD          (:372-390, 415-439)
 *   G M, G V     the same times the particle mass / fall speed (:393-412, :457-478)
 * so that N(D_k) = G exp(-lambda_r D_r): everything that depends on the wet fraction only
 * (two cube roots, a sixth / fourth root, two powers for graupel, a division per bin) is read
 * from the table; the rain slope lambda_r stays per item.
 * 1-moment ice with tab_degree = CPOL_ICE_DEGREE (and uniform_grid): the aux block of the
 * recurrence form (4 n_d + 8 + 8 n_d values) is followed by [log2(lambda_lo), panels per octave,
 * n_panels, 0] and [n_panels][CPOL_ICE_FUNCS][CPOL_ICE_DEGREE + 1] monomial coefficients in
 * u in [-1, 1] across a panel of log2(lambda): the renormalisation sums of IceParticle.set_psd /
 * integrate_V (hydrometeors.py:1331-1339, 1256-1275) are 1024-term sums that depend on the
 * item's lambda only, not on its LUT slice. */
CPOL_API int  cpol_stage_hydro(cpol_ctx *ctx, int slot, const cpol_hydro_desc *desc,
                      const double *table, const double *pre, const double *dnu,
                      const double *aux, int n_aux);
CPOL_API int  cpol_set_num_hydro(cpol_ctx *ctx, int n_hydro);
/* Finishes staging: builds the INTEGRAL TABLES now instead of at the first sweep / cpol_fork.
 * For every species whose N(D) has one per-item shape parameter lambda (all gamma-family species,
 * 1-moment ice) the 12 PSD-integrated entries of an item -- what get_N + lookup_line + einsum
 * (hydrometeors.py:128-147, lut.py:309-344, doppler_scatter.py:246-251) produce -- are a per-item
 * scale times a function of (LUT slice, lambda) only.  The integrating kernels evaluate that
 * function once per (slice, 1/8-octave panel of lambda, Chebyshev node) and store degree-10
 * polynomials ("1-D blocks": 11 rows of 16 float64 per (slice, panel)); a sweep then gathers
 * 12 x 11 coefficients per item instead of integrating 1024 diameter bins.
 * The melting species (wet fraction fw and rain-partner slope lambda_r) get "2-D blocks": per (slice,
 * 1/4-octave panel of lambda_r) the polynomial of total degree 10 in (fw inside the slice's wet-
 * fraction bin, position inside the panel), 66 rows of 16 float64; a sweep evaluates 14 functions
 * (12 columns + 2 Doppler sums) per item.
 * ACCURACY GATE: every block carries one more item at an off-node point, integrated by the same
 * kernel and compared with the polynomial function by function on the scale of the function over
 * the block.  1-D tables keep the longest run of lambda panels whose blocks all stay below 1e-10
 * (in practice all but the last panel, where exp(-lambda D^nu) of the bins behind the first goes
 * subnormal); a 1-D table with less than half of its panels left, and a 2-D table with any block
 * above 1e-10, is dropped.  Items outside the accepted ranges are integrated bin by bin as in round
 * 1.  cpol_debug_read("itab_check"): per slot the worst accepted deviation (negative: table dropped;
 * 0: none), then where it was found, then the number of (block, function) pairs above the limit;
 * "itab_detail<slot>": per lambda panel and per function; "itab_times": device ms of build / gate.
 * Environment (read at every build): CPOL_ITAB=0 no tables at all, CPOL_ITAB_MELT=0 none for the
 * melting species, CPOL_ITAB_MAX_DEV=<x> another limit than 1e-10.  (Read by cpol_create: CPOL_SUBSUM=0;
 * per sweep: CPOL_LOOKUP_TILE=0, see INTEGRATION.md.)
 * COST: a few ms of kernels per gamma / ice slot, ~90 ms per melting slot on full-size tables
 * (46 x 100 slices); TRANSIENT device memory of the build = n_e * n_t * n_panels * 12 (1-D) or
 * * 122 (2-D) synthetic items x ~164 B: 1 GB for a gamma slot, ~3.5 GB for a melting slot of that
 * size; RESIDENT tables 0.3 - 0.5 GB per 1-D slot, 1.5 GB per melting slot.
 * Depends on every staged table: call after the last cpol_stage_* (any later staging call
 * invalidates the tables; they are rebuilt on demand). */
CPOL_API int  cpol_prepare(cpol_ctx *ctx);

/* float32 functions of the gate temperature, TABULATED BY THE HOST over every float32 value
 * in [128 K, 512 K) (2^24 consecutive bit patterns from CPOL_TFUN_FIRST_BITS).  The reference
 * evaluates them with NumPy's float32 exp / power, which are not correctly rounded (1-2 ulp off
 * in 20-40 % of the arguments); a 1-ulp difference in the snow intercept becomes > 1e-5
 * relative in K_DP, a difference of near-equal float32 sums.  The host evaluates the
 * reference's own expressions with its own NumPy, the device looks the value up by the bit
 * pattern of T: the bits the reference would have used, on every host.  Optional: without a
 * table (or outside the range) the device computes the correctly rounded value.
 *   CPOL_TFUN_SNOW_N0     13.5*(5.65e5*exp(-0.107*(T-273.15)))/1000   hydrometeors.py:896
 *   CPOL_TFUN_ICE_MOM2_A  10**a(T - 273.15), Field et al. (2005)      hydrometeors.py:1287-1292 */
enum { CPOL_TFUN_SNOW_N0 = 0, CPOL_TFUN_ICE_MOM2_A = 1, CPOL_N_TFUN = 2 };
#define CPOL_TFUN_FIRST_BITS 0x43000000u      /* 128.0f */
#define CPOL_TFUN_COUNT      (1u << 24)       /* every float32 in [128, 512) */
CPOL_API int  cpol_stage_t_function(cpol_ctx *ctx, int which, const float *table /* [CPOL_TFUN_COUNT] */);

/* Doppler scheme 2 (doppler_scatter.py:283-296): per table slice and diameter bin the
 * trapezoid weight w_k (1/2 at both ends) times the horizontal radar cross-section
 * 2 pi (Z11 - Z12 - Z21 + Z22), and the same times the fall speed V(D_k):
 * weights [n_e][n_t][n_d][2] = (w rcs V, w rcs) float64.  Needed only when
 * cpol_sweep_params.simulate_doppler == 2. */
CPOL_API int  cpol_stage_doppler_weights(cpol_ctx *ctx, int slot, const double *weights);

/* Doppler scheme 3: per table slice and diameter bin the float32 horizontal radar cross
 * section 2 pi (Z11 - Z12 - Z21 + Z22) (doppler_scatter.py:686-695), and the float32
 * diameter grid np.linspace(d_min, d_max, n_d) of get_doppler_spectrum with D^mu, D^nu
 * evaluated in float32 (:676-681): dgrid = [3][n_d].  Power-law species only. */
CPOL_API int  cpol_stage_spectrum_tables(cpol_ctx *ctx, int slot, const float *rcs32, const float *dgrid);

/* gate kernel on explicit points: coords [n][2] (rotated lat, lon) float32,
 * heights [n] float32 -> out [n_vars][n] float32 with the reference's
 * sentinels (-9999 above the model top, NaN below topography). */
CPOL_API int  cpol_interp_points(cpol_ctx *ctx, int n, const float *coords, const float *heights,
                        float *out);

/* The filter of the Doppler-spectrum broadening on explicit rows (the device function the sweep runs, one row per
 * workgroup): rows [n_rows][n_v] float32, sigma_bins [n_rows] float64 (standard deviation in bins) -> out [n_rows][n_v]
 * float32 = scipy.ndimage.gaussian_filter(row, sigma) (truncate 4, mode 'reflect', any radius), rescaled to the float32
 * sum of the input row; a row without power becomes NaN; sigma <= 1e-15 or NaN filters as the identity.  Host
 * buffers; n_v in [2, 4097].  Needs no staged model or tables. */
CPOL_API int  cpol_broaden_rows(cpol_ctx *ctx, const float *rows, int n_rows, int n_v, const double *sigma_bins,
                       float *out);

/* fills per-ray tables with libm (C callers); Python callers use numpy.
 * traj_out: [n_rays][n_vnodes][CPOL_TRAJ_STRIDE] doubles (el_rad, sin el, cos el, el_deg);
 * geo_out:  [n_rays][n_hnodes][CPOL_GEO_STRIDE] doubles. */
CPOL_API int  cpol_ray_tables(const cpol_sweep_params *p, const double *az_deg, const double *el_deg,
                     const double *pts_h_deg, const double *pts_v_deg,
                     double *traj_out, double *geo_out);

CPOL_API int  cpol_run_sweep(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_ray_tables_t *tables,
                    cpol_outputs *out);

/* Sub-beam columns of cpol_interp_subbeams: every array [n_rays][n_sub][n_gates] (the library's own sub-beam order),
 * NULL = not wanted.  Host buffers, or device buffers with outputs_on_device = 1. */
typedef struct {
    float   *vals;              /* [n_vars][...] float32 model values (after the melting scheme unless skipped)      */
    int8_t  *mask;              /* mask codes (-1 below the topography, 0, 1 above the model top, 2 outside the domain) */
    float   *elev;              /* elevation [deg] as get_interpolated_radial leaves it (not folded)                 */
    double  *lats, *lons;       /* gate coordinates of every sub-beam (the long form of the geodesy)                */
    float   *dist, *heights;    /* distance at the ground and height [m]                                             */
    float   *q_melt;            /* [2][...] QmS_v, QmG_v (melting.py:19-90; zero where nothing melts)                */
    double  *fw_melt;           /* [2][...] fwet_mS, fwet_mG                                                        */
    int8_t  *mask_ml;           /* the reference's mask_ml: QR > 0 and QS + QG > 0 before melting; has_melting = any
                                   over a sub-beam                                                                    */
    double  *wgate;             /* integration scheme 'ml' (tables->sub_smooth): the per-gate sub-beam weights        */
    int32_t skip_melting;       /* 1: no melting scheme (raw interpolated values; q_melt / fw_melt / mask_ml unwritten) */
    int32_t outputs_on_device;  /* 1: the pointers above are device memory and the call returns at once             */
} cpol_subbeam_outputs;

/* The first half of cpol_run_sweep for the same rays: ray paths, gate geodesy, gate interpolation (the sweep's own
 * forms: the values carry cpol_run_sweep's bits) and, unless out->skip_melting, the melting scheme -- the reference's
 * get_interpolated_radial (interpolation/interpolation.py:91) for every ray.  No scattering.  p->with_melting selects
 * the melting scheme as for the sweep; apply_sensitivity / integrate_model are ignored.  Needs a staged model and
 * staged hydrometeors. */
CPOL_API int  cpol_interp_subbeams(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_ray_tables_t *tables,
                      cpol_subbeam_outputs *out);

/* Sub-beam columns supplied by the caller (cpol_run_columns): the input of the reference's get_radar_observables
 * (scatter/doppler_scatter.py:49) for n_rays radials of n_sub sub-radials each.  Per-gate arrays are
 * [n_rays][n_sub][n_gates], the library's own sub-beam order. */
typedef struct {
    int32_t n_vars;             /* entries of `vals`: the variable order the staged hydrometeor descriptors (var_q,
                                   var_t, var_qn) and cpol_sweep_params.var_u / var_v / var_w / var_rho index */
    int32_t inputs_on_device;   /* 1: the per-gate arrays and has_melting are device pointers (read in place, never
                                   written); 0: host memory.  The per-ray tables below are always host memory */
    const float *const *vals;   /* [n_vars] per-gate float32 model values (the pointer array itself is host memory).
                                   With q_melt: after the melting scheme (QR / QS / QG zeroed where it melted) */
    const int8_t *mask;         /* per-gate mask codes (-1, 0, 1, 2) or NULL (all 0); feeds the radial mask only */
    const float *elev;          /* per-gate elevation [deg], unfolded or folded: folded on the device (Q8) */
    const double *wgate;        /* per-gate sub-beam weights (integration scheme 'ml') or NULL: sub_w        */
    const float *q_melt;        /* [2] x per-gate QmS_v, QmG_v given by the caller, or NULL: with_melting = 1
                                   diagnoses melting on the device from QR / QS / QG as cpol_run_sweep does */
    const double *fw_melt;      /* [2] x per-gate fwet_mS, fwet_mG (with q_melt)                            */
    const int8_t *has_melting;  /* [n_rays][n_sub] 0: the given melting fields of that sub-beam count as zero
                                   (doppler_scatter.py:160-165), or NULL (all 1); only with q_melt        */
    /* per-ray tables (host) */
    const double *az_sincos;    /* [n_rays][n_sub][2] sin and cos of each sub-beam's azimuth (the first two entries
                                   of the sweep's `geo` table); needed with simulate_doppler                */
    const double *sub_w;        /* [n_sub] quadrature weights (required)                                     */
    const double *nyquist;      /* [n_rays] or NULL, as in cpol_ray_tables_t                                 */
    const double *sens_thr;     /* [n_gates] or NULL, as in cpol_ray_tables_t                                */
    const double *varray;       /* [n_vbins] (Doppler scheme 3) or NULL                                     */
} cpol_columns_t;

/* The second half of cpol_run_sweep on caller-supplied sub-beam columns: PSD, scattering, sub-beam sums, ZH ... RVEL
 * and the sensitivity cut, into the same cpol_outputs struct; lats / lons / dist / heights are not written (the columns carry
 * no geometry).  p: n_rays, n_gates, n_sub and the radar / scheme fields as for cpol_run_sweep; n_hnodes, n_vnodes,
 * geometry_mode and the site fields are ignored.  Needs staged hydrometeors, no staged model; works on a lane.
 * CPOL_ERR_ARG (the context stays usable) on bad shapes, a missing variable pointer, a descriptor index >= n_vars,
 * n_gates > CPOL_MAX_GATES (as for cpol_run_sweep: refused before anything is queued) or mask_sum8 with 2 * n_sub > 127. */
CPOL_API int  cpol_run_columns(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_columns_t *cols,
                      cpol_outputs *out);

/* One scan over MANY members (replaces in the reference: nothing -- it runs one model state per process).  The ray paths,
 * the geodesy, the rotated-pole transform, the grid cell and the level search of every sub-beam gate are evaluated ONCE
 * (k_interp_members: in the forms cpol_run_sweep takes for the same rays), the variables of every requested member are
 * gathered and interpolated behind them, and the second half of the launch sequence runs over n_members * n_rays rows (row
 * m * n_rays + r = ray r of members[m]) as cpol_run_columns runs it: no interpolating forms, no graph replay
 * ("launch_forms" reports them).  Every member's arrays carry the bits of cpol_run_sweep after cpol_select_member.
 * members: n_members distinct staged member indices in any order, at most 64 per call.  p and tables: as for cpol_run_sweep
 * (n_rays = the rays of ONE member).  out: the per-gate arrays are [n_members][n_rays * n_gates] (sz_total, DSPECTRUM and
 * mask_sum8 likewise); lats, lons, dist and heights are [n_rays * n_gates], once; model_vars must be NULL (p->integrate_model is
 * ignored).  All three outputs_on_device modes; works on a lane; the context's selected member is not changed.
 * CPOL_ERR_ARG (the context stays usable): a member not staged or listed twice, model_vars requested, mask_sum8 with
 * 2 * n_sub > 127, more than 2^31 - 1 sub-beam gates in all.  Work memory: cpol_mem_info's per_gate x n_members per sub-beam gate.
 *
 * TIME BLEND (tables->time_blend = 1; replaces in the reference: nothing -- it reads one model state, at its own time).  ONE scan of
 * p->n_rays rays whose ray r sees the model between two staged states: `members` lists the states the call may read (at most
 * 64, in the order of the series; a state may be listed twice), tables->ray_state[r] is the index INTO `members` of the earlier
 * state and tables->ray_weight[r] the float32 weight w of the later one, members[ray_state[r] + 1].  Every one of the eight
 * neighbour values of a sub-beam gate is blended per staged variable in float32 -- w == 0: a, the later state is not read;
 * otherwise a + w * (b - a), three operations in that order; -9999 where a or b is -9999 -- before the vertical
 * interpolation (k_interp_timed: the geometry once per sub-beam gate, in cpol_run_sweep's forms), so every output carries the
 * bits of cpol_run_sweep on a context staged with the cube blended that way on the host.  out: the shapes of cpol_run_sweep,
 * [n_rays * n_gates]; model_vars and p->integrate_model are honoured.  Work memory: per_gate x 1.  The second half runs over
 * n_rays rows under the rules above (no interpolating forms, no graph replay).  All three outputs_on_device modes; works on
 * a lane; the selected member is not changed.  CPOL_ERR_ARG (the context stays usable, nothing is queued): ray_state or
 * ray_weight NULL, a ray_state outside `members`, ray_state + 1 outside it with a weight != 0, a weight outside [0, 1) or not
 * finite, CPOL_GEOM_SPACEBORNE or CPOL_GEOM_HOST_PATHS. */
CPOL_API int  cpol_run_sweep_members(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_ray_tables_t *tables,
                            const int32_t *members, int n_members, cpol_outputs *out);

/* CPOL_GEOM_SPACEBORNE helper: index of the first candidate gate below the
 * model-top ceiling for each (ray, vertical node): first_gate [n_rays*n_vnodes]
 * (host buffer).  `traj` [n_rays][n_vnodes][CPOL_TRAJ_STRIDE] and `site`
 * [n_rays][CPOL_SITE_STRIDE] as in cpol_ray_tables_t, n_cand[n_rays] candidate gates. */
CPOL_API int  cpol_spaceborne_first_gate(cpol_ctx *ctx, const cpol_sweep_params *p, const double *traj,
                                const double *site, const int32_t *n_cand, double ceiling_m,
                                int32_t *first_gate);

CPOL_API int  cpol_counters(cpol_ctx *ctx, cpol_counters_t *out);
/* on = 1: HIP events around every stage of every sweep (7 per sweep); on = 2: only around the
 * PSD x table stage (2 per sweep; ms_psd alone is filled in); on = 0: off */
CPOL_API int  cpol_enable_timing(cpol_ctx *ctx, int on);

/* debug / parity access to intermediate device buffers of the last sweep:
 * "sub_values" float32 [n_vars][n_sbg], "sub_mask" int8 [n_sbg], "sub_elev"
 * float32 [n_sbg], "sub_coords" float32 [n_sbg][2], "item_key" int32
 * [n_hydro][n_sbg], "sz_integ" float32 [n_rays*n_gates][n_hydro][12],
 * "traj" float32 [n_rays][n_vnodes][3][n_gates], "item_res" float64
 * [n_hydro][n_sbg][12], "sub_wgate" float64 [n_sbg] (integration scheme 'ml': the per-gate
 * sub-beam weights), "geo_poly" float64 [n_rays][n_hnodes][2][9] (a test hook: the coordinate polynomials the gate
 * kernel of the last sweep read -- monomial coefficients of the rotated latitude, then longitude, in x = 2 s / s_max - 1; NaN: a fit
 * that k_trajectory's sanity rules rejected; CPOL_ERR_ARG after a sweep that took none); after a sweep in the general launch sequence (refused after the single-beam
 * kernels, which do not write them for every gate) "item_vmask" uint8 [n_sbg] (bit j: hydrometeor j valid)
 * and, under Doppler scheme 1, "item_vn" float64 [n_hydro][n_sbg][2] -- the fall-speed sums {v, n} of every
 * item, defined where its bit of "item_vmask" is set -- and, when a species' sums are totals over the ray
 * (1-moment ice, numeric integrate_V), "ice_first" [n_rays * n_sub] records {int32 first_gate (0x7fffffff: none), int32 pad,
 * float64 v, float64 n}.  Without the debug reads enabled: "launch_forms" int32 [12] -- which launch
 * sequence the last cpol_run_sweep of this context took: [0] the CPOL_GATE1_RAY rule in force,
 * [1] k_gate1_ray ran, [2] the single-beam gate kernel, [3] k_interp_classify, [4] items off the
 * tables listed directly, [5] k_subbeam_sum, [6] table items evaluated in place, [7] the one
 * sub-beam on the coordinate polynomials, [8] n_sub, [9] lanes alive, [10] the build's CPOL_SCAN_FORM (1: wavefront range scans), [11] a HIP
 * graph was replayed; "poly_central", "host_times", "cache", "itab_check", "itab_times",
 * "itab_detail<slot>" (see cosmo_pol_amd/_native.py); the staged model as it lies in device memory: "model_v" float32
 * [ny][nx][nz][n_vars], "model_h" float32 [ny][nx][nz], "model_ht" float32 [ny][nx][2] (model top, lowest level);
 * "ingest_times" float64 [4]: milliseconds of the last packed staging (octets to the device, k_grib_unpack,
 * k_model_derive, the whole call).
 * Gate stencils (single-beam sweeps under a caller's table version: from the third sweep of a geometry over unchanged level
 * heights the gate kernel replays its ray paths, grid cells and bracketing levels from a per-gate record instead of
 * computing them; bit-identical outputs): "stencil" float64 [6] -- the form of this context's last sweep (0 full, 1 recording,
 * 2 replay), then of the root context's store: entries, bytes held, records made, replays, entries dropped.
 * "stencil_budget" is a CONTROL name like "enable": dst points to a uint64, the bytes the store may hold (0: stencils off;
 * default 1 GiB).  Root context only and refused (CPOL_ERR_ARG) while lanes of it exist; lowering it below what is held drops
 * every entry.  Returns 0.
 * "terrain_shadow_rows" is a CONTROL name too, a test hook in the manner of cpol_debug_scan: k_terrain_shadow alone on caller
 * arrays.  dst points to { int32_t n_rows, n_gates, n_vars, pad; int8_t *mask; float *vals; } -- host arrays, `mask`
 * [n_rows][n_gates] codes and `vals` [n_vars][n_rows * n_gates], both shadowed in place by the rule of "Terrain shadowing" above;
 * blocking; needs no staged model.  CPOL_ERR_ARG: a NULL pointer, n_rows / n_gates < 1, n_vars outside 1 .. CPOL_MAX_VARS,
 * n_rows * n_gates >= 2^31.  Returns 0.
 * "superob_fields" is a CONTROL name too, a test hook: k_superob on caller-supplied per-gate arrays.  dst points to
 * { int32_t n_rows, n_gates; const void *in[10]; cpol_superob so; } -- `in` in the order of cpol_superob.count's rows, host arrays
 * [n_rows * n_gates] float32 (slot ZDR unused, slot RVEL float64, NULL = not given), `so` with host output pointers
 * (rays_per_block = 0: n_rows); blocking; cpol_superob's refusals, and CPOL_ERR_ARG for a requested field without its input.
 * Returns 0.
 * "member_stats_fields" is its sibling for the ensemble statistics: k_member_fold / k_member_finish / k_member_quantile and the
 * context's running state on caller-supplied members.  dst points to { int32_t n_members; int64_t n_cells; const void *in[10]; cpol_member_stats
 * ms; } -- `in[k]` a host array [n_members][n_cells] (float32, slot RVEL float64; needed for every folded field when n_members
 * > 0; n_members = 0 folds nothing), `ms` with host output pointers; blocking; honours ms.phase, so a pass can be cut into
 * calls; cpol_member_stats' refusals (Doppler counts as on).  Returns 0.
 * "member_verify_fields" is the same hook with a verification beside it (k_member_verify): dst points to { int32_t n_members;
 * int64_t n_cells; const void *in[10]; cpol_member_stats ms; cpol_member_verify mv; } -- `mv` with host observation and output
 * pointers; blocking; honours ms.phase; cpol_member_stats' and cpol_member_verify's refusals.  Returns 0.
 * "spectrum_moments_rows" is the sibling for the spectrum moments: k_spec_moments on caller-supplied spectra.  dst points to
 * { int32_t n_rows, n_v; const double *spectrum; const double *varray; cpol_spectrum_moments sm; } -- host arrays, `spectrum`
 * [n_rows][n_v], every row treated as a gate, `varray` [n_v], `sm` with host output pointers sized for n_rows gates; blocking;
 * needs no staged model or tables; cpol_spectrum_moments' refusals (Doppler scheme 3 counts as on), and CPOL_ERR_ARG for
 * n_rows < 1, n_v outside 1..4097 or a NULL input.  Returns 0.
 * "histogram_fields" is the sibling of "superob_fields" for the sweep histograms: k_hist and the context's running state on
 * caller-supplied rows.  dst points to { int32_t n_rows, n_gates, n_rays, n_model_vars; const void *in[10]; const float *heights,
 * *dist; const double *model_vars; cpol_histogram h; } -- host arrays: `in` in the order of the fields, [n_rows * n_gates]
 * float32 (slot RVEL float64), needed for every requested field and for a field taken as ordinate; heights and dist
 * [n_rays * n_gates] (n_rays divides n_rows: row r takes row r mod n_rays); model_vars [n_model_vars][n_rows * n_gates]; `h` with
 * host edge and output pointers; blocking; honours h.phase; needs no staged model or tables; cpol_histogram's refusals (Doppler
 * counts as on), and CPOL_ERR_ARG for a bad shape or a missing input.  Returns 0.
 * "histogram_stretch" copies one int32: the gates a workgroup of k_hist owns.
 * "species_fields" is the same for the hydrometeor contributions: k_species alone on caller-supplied rows.  dst points to
 * { int32_t n_rows, n_gates; const float *sz; const float *zh_final; float c_zh, c_kdp, c_2w, pad_; cpol_species sp; } -- host
 * arrays: sz [n_rows * n_gates][sp.n_hydro][12], zh_final [n_rows * n_gates]; `sp` with host output pointers (sp.sz: the rows
 * back from the device); blocking; needs no staged model or tables (n_hydro is the hook's own, 1 ... CPOL_MAX_HYDRO);
 * CPOL_ERR_ARG for a bad shape, a NULL input or every output NULL.  Returns 0.
 * "composite_fields" is the same for the gridded composites: the plan, the placement, k_comp, k_comp_finish and the context's
 * running state on caller-supplied rows.  dst points to { int32_t n_rows, n_gates, n_rays, lane_form; const float *in[9];
 * const float *heights, *dist; cpol_composite c; } -- host arrays: `in` in the order of the fields, [n_rows * n_gates] float32,
 * needed for every requested field; heights and dist [n_rays * n_gates] (n_rays divides n_rows: row r takes row r mod n_rays);
 * `c` with host edge, ray and output pointers (ray_sin, ray_cos [n_rays]); lane_form 0: the kernel's kept form, 1: lanes that
 * share a cell combined inside the wavefront, 2: every lane on its own; blocking; honours c.phase; needs no staged model or
 * tables; cpol_composite's refusals, and CPOL_ERR_ARG for a bad shape or a missing input.  Returns 0.  With c.plane =
 * CPOL_COMP_PLANE_GATES c.gate_x and c.gate_y are host arrays [n_rays * n_gates] (kept under c.plane_version like a sweep's) and
 * dist may be NULL; with CPOL_COMP_SOURCE in c.products the call runs k_comp_merge too, with c.source.  With height layers
 * (c.n_z > 0) the call runs the layered k_comp, and a finishing call with CPOL_COMP_COLUMN runs k_comp_column and copies
 * c.column / c.column_layers (host arrays) too.  With CPOL_COMP_SUM in c.products `c` is the member `c` of a cpol_composite_sums,
 * the last member of the hook's struct (max_bytes covers it): the call runs k_comp_sum behind k_comp (lane_form: 0 the kept form,
 * 1 the runs of a wavefront summed first, 2 every lane on its own) and a finishing call k_comp_sum_finish, and copies sum /
 * sum_skipped (host arrays) too.  Without the bit the hook takes and returns exactly what it did.
 * "composite_plane" copies two int64: {uploads, hits} of the context's store of gate planes (cpol_composite.plane_version).
 * "composite_stretch" copies one int32: the gates a workgroup of k_comp owns.
 * "fractions_maps" is the same for the neighbourhood verification: the checks and the three kernels of cpol_frac.inl on
 * caller-supplied maps.  dst points to { int32_t n_blocks, n_y, n_x, pad; const float *maps; cpol_fractions f; } -- host arrays:
 * maps [n_blocks][n_y][n_x] float32 (what a finished plane would hold; f.field and f.plane are not read), f.observed, f.domain
 * (or NULL), f.sums and f.totals; 1 <= n_x, n_y <= 1023; blocking; needs no staged model, tables or composite pass;
 * cpol_fractions' refusals, and CPOL_ERR_ARG for a bad shape or NULL maps.  Returns 0.  With f.objects (host arrays n_objects,
 * table and labels or NULL) the call runs cpol_objects' checks and the kernels of cpol_obj.inl on the same maps too; with a
 * non-zero f.objects->pad_ the struct is the first member of a cpol_objects_match, whose n_pieces, pieces and covered are host
 * arrays, and the match runs as well.  With CPOL_FRAC_ENSEMBLE in f.n_radii a pointer to a cpol_fraction_probabilities follows
 * f (the two are a cpol_fractions_ensemble; max_bytes covers it; host arrays prob_sums, reliability, and member_sum, member_any
 * or NULL), and the call runs its checks and k_frac_members on the same maps too.
 * Returns bytes copied or < 0. */
CPOL_API int64_t cpol_debug_read(cpol_ctx *ctx, const char *name, void *dst, int64_t max_bytes);

/* test hook: evaluates one of the device math helpers of the melting-species kernel on
 * host arrays (op 0 exp, 1 log, 2 cbrt, 3 cbrt via x^(-1/6), 4 x^(1/6), 5 x^(1/4), 6 1/x; 7: float32 pairs (n, d) in
 * the words of x, 0 where the reciprocal division has the bits of n / d; 8: the attenuation factor of a gate as the
 * kernels form it, (float)exp10((double)x) of a float32 x held in the double, the float32 result as a double) */
CPOL_API int  cpol_debug_math(cpol_ctx *ctx, int op, const double *x, double *y, int n);

/* test hook: the range-scan functions of the kernels themselves on n_rows rows of n float32 (host arrays x -> y, row
 * after row): one workgroup per row copies it into LDS, runs the running sum (mul = 0) or product (mul != 0) of the
 * wavefront form (form 1: the shifted adds / multiplies the sweeps use) or the one-lane loop (form 0), and copies it
 * back.  CPOL_ERR_ARG: form not 0 / 1, n_rows < 1 or > 65535, n < 1 or n > 16384 (a row in 64 KB of LDS). */
CPOL_API int  cpol_debug_scan(cpol_ctx *ctx, int form, int mul, const float *x, float *y, int n_rows, int n);

#ifdef __cplusplus
}
#endif
#endif
