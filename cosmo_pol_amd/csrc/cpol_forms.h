// cpol_forms.h -- which kernels a sweep launches, and in which template form: every launch rule of run_sequence
// (cosmo_pol_hip.hip), decided once per call by choose_forms() from plain numbers.  Plain C++ without HIP types, so that a
// host test can include it (tests/c_host/forms_check.cpp, tests/test_forms_cpu.py pin the rules without a GPU).  The
// measurement notes beside a rule are the record of why it exists.  Grid and LDS sizes stay with the launches.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "../../include/cosmo_pol_amd.h"

// build constants of the kernel files that the rules read (cosmo_pol_hip.hip asserts each against its kernel file)
constexpr int FORMS_RAY_PREP_MIN_SUB = 4;      // CPOL_RAY_PREP_MIN_SUB (cpol_interp.inl)
constexpr int FORMS_TILE_GATES_LOG2 = 2;       // CPOL_TILE_GATES_LOG2 (cpol_psd.inl): a wavefront of k_psd_lookup / k_subbeam_sum = 16 rays x 4 gates
constexpr int FORMS_FINAL_THREADS = 256;       // CPOL_FINAL_THREADS (cpol_final.inl)
enum { FORMS_MODE_GAMMA_EXP = 0, FORMS_MODE_GAMMA_UNIFORM = 1, FORMS_MODE_ICE = 2, FORMS_MODE_MELTING = 3 };     // PSD_MODE_* (cpol_psd.inl)

// ---- knobs of a context: read when it is created (cpol_create), copied to its lanes (cpol_fork) ----
struct Knobs {
    // CPOL_USE_GRAPH=1 (opt-in): replaying the captured sequence cuts the host time of a sweep 4x (0.12 -> 0.03 ms) but is no
    // faster on the device (0.232 vs 0.222 ms single lane) and slows three-lane throughput by a quarter when graph launches
    // and plain launches mix
    bool use_graph = false;
    int subsum_coop_rounds = 6;        // CPOL_SUBSUM_COOP_ROUNDS: scalar-cache rounds per wavefront and sub-beam before the gather tail
    int rare_overlap = 0;              // CPOL_RARE_OVERLAP=1: k_psd_rare beside k_psd_lookup on a sibling stream instead of behind it (measured: the share of
                                       // one of 8 GPUs 1.42 -> 1.37 ms alone, 0.97 -> 0.99 with three lanes; the C3 sweep 151 -> 167 us: the fork and join cost
                                       // more than the idle launch -- off)
    int rare_direct = 1;               // CPOL_RARE_DIRECT=0: keep the counting sort of the items outside the tables
    int lookup_list = 1;               // CPOL_LOOKUP_LIST=0: k_psd_lookup starts one wavefront per tile instead of workgroups that list the tiles with work among their own; 2: the list for every launch size
    int lookup_split = 0;              // CPOL_LOOKUP_SPLIT=<n>: wavefronts per tile of k_psd_lookup (0: by launch size)
    int gate1_ray = -1;                // -1 (default): 1 in a context with lanes (sweeps in flight side by side: three launches instead of four per sweep are 6-8 % of
                                       // c2's throughput), 0 without (the isolated sweep: 88 against 91 us); CPOL_GATE1_RAY=0: never; 1: k_gate1_ray (items off the tables integrated in place, the range scans by k_scan_rays: a single-beam sweep
                                       // of three lean launches, no integrating launch); 2: also with tables that lost panels; 3: the scans inside the gate kernel (a ticket per ray)
    int gate1_species = 1;             // CPOL_GATE1_SPECIES=0 / 2: never / always k_gate1_species (one wavefront per species; default: small launches)
    int fuse_gate1 = 0;                // CPOL_FUSE_GATE1=1: k_interp_gate1 instead of k_interp_sweep + k_gate1 (measured slower where it matters)
    int fuse_classify = 1;             // CPOL_FUSE_CLASSIFY=0: k_interp_sweep + k_classify instead of k_interp_classify
    int gate1 = 1;                     // CPOL_GATE1=0 / 2: never / also with melting species: the single-beam fused kernel
    int subsum = 1;                    // CPOL_SUBSUM=0: the plain form: k_psd_lookup stores every item's columns and one thread of k_final walks the sub-beams in order
    int subsum_scalar = 0;             // CPOL_SUBSUM_FORM=scalar: the cooperative form of k_subbeam_sum takes its rows through the scalar cache instead of LDS
    int upload_kernel = 0;             // CPOL_TABLE_UPLOAD=kernel: the per-ray tables by k_upload_tables instead of hipMemcpyAsync (a measurement knob)
    int geo_poly_central = 1;          // CPOL_GEO_POLY_CENTRAL=0: a single-beam sweep keeps the long form of the geodesy for its (central) sub-beam even when
                                       // nobody asks for the float64 latitude / longitude; 2: the polynomials also with the debug reads enabled (tools/fast_sub_check.py)
    int geo_poly = 1;                  // CPOL_GEO_POLY=0: the non-central sub-beams take the short closed form of the geodesy instead of the per-ray polynomials
    int psd_rare = 1;                  // CPOL_PSD_RARE=0: one launch per integrating flavour also when the units are directly listed items
    int subsum_small = 0;              // CPOL_SUBSUM_SMALL=1: experiment: the gather form of k_subbeam_sum with three wavefronts per (tile, hydrometeor) and the whole block in flight (measured slower)
    int subsum_chain = 1;              // CPOL_SUBSUM_CHAIN=0: the team's terms pass through LDS and a barrier per round instead of its float32 sums waiting in LDS, handed
                                       // from sub-beam to sub-beam (share of one of 8 GPUs: 385 against 334 us)
    int subsum_team = -1;              // CPOL_SUBSUM_TEAM=W: k_subbeam_sum_team<W> (W = 2..8 wavefronts per (tile, species)) for every launch; 0: never (the one-wavefront
                                       // forms alone); -1 (default): W = 4 for the launches too small for the LDS form
    int subsum_coop = -1;              // CPOL_SUBSUM_COOP: k_subbeam_sum takes its coefficients cooperatively (LDS / scalar cache): 0 never, 1 always, -1 by launch size (the results are identical)
};

inline Knobs knobs_from_env()
{
    Knobs k;
    const auto num = [](const char *name, int &v) { const char *e = getenv(name); if (e) v = atoi(e); return e != nullptr; };
    const auto flag = [&](const char *name, int &v) { if (num(name, v)) v = v != 0 ? 1 : 0; };
    const auto clamp = [&](const char *name, int &v, int lo, int hi) { if (num(name, v)) v = std::max(lo, std::min(hi, v)); };
    int g = 0;
    flag("CPOL_USE_GRAPH", g);
    k.use_graph = g != 0;
    flag("CPOL_SUBSUM_COOP", k.subsum_coop);
    clamp("CPOL_LOOKUP_LIST", k.lookup_list, 0, 2);
    clamp("CPOL_LOOKUP_SPLIT", k.lookup_split, 0, 16);
    clamp("CPOL_GATE1_SPECIES", k.gate1_species, 0, 2);
    clamp("CPOL_GATE1_RAY", k.gate1_ray, -1, 3);
    flag("CPOL_FUSE_GATE1", k.fuse_gate1);
    flag("CPOL_FUSE_CLASSIFY", k.fuse_classify);
    flag("CPOL_RARE_OVERLAP", k.rare_overlap);
    flag("CPOL_RARE_DIRECT", k.rare_direct);
    num("CPOL_GATE1", k.gate1);
    flag("CPOL_SUBSUM", k.subsum);
    if (getenv("CPOL_SUBSUM_FORM")) k.subsum_scalar = !strcmp(getenv("CPOL_SUBSUM_FORM"), "scalar") ? 1 : 0;
    flag("CPOL_SUBSUM_CHAIN", k.subsum_chain);
    num("CPOL_SUBSUM_TEAM", k.subsum_team);
    flag("CPOL_SUBSUM_SMALL", k.subsum_small);
    if (getenv("CPOL_TABLE_UPLOAD")) k.upload_kernel = !strcmp(getenv("CPOL_TABLE_UPLOAD"), "kernel") ? 1 : 0;
    clamp("CPOL_GEO_POLY_CENTRAL", k.geo_poly_central, 0, 2);
    flag("CPOL_GEO_POLY", k.geo_poly);
    flag("CPOL_PSD_RARE", k.psd_rare);
    clamp("CPOL_SUBSUM_COOP_ROUNDS", k.subsum_coop_rounds, 0, 64);
    return k;
}

// ---- experiment knobs of the process: read once, at the first sweep (tests/test_gpu_boundary.py and tools/psd_flavours.py
// set them in a child's environment) ----
struct ProcessKnobs {
    int gate1_present = 1;             // CPOL_GATE1_PRESENT=0: k_gate1_ray without the presence words (a build with CPOL_GATE1_PRESENT alone writes them)
    int exp_skip = 0;                  // CPOL_EXP_SKIP, timing experiments only -- wrong results: bit 0 the gate interpolation, bit 1 k_gate1_ray, bit 2 the scans
    int lookup_tile = 1;               // CPOL_LOOKUP_TILE=0: k_psd_lookup by sub-beam gate instead of ray x gate tiles
    long lookup_fill = 12;             // CPOL_LOOKUP_FILL: how many times over the listing workgroups of k_psd_lookup fill the chip (C4 volume, 1 / 3 / 6 / 12 / 24 / 48: 1.28 / 1.25 / 1.24 / 1.20 / 1.23 / 1.26 ms)
    int ice_force_sum = 0;             // CPOL_ICE_FORCE_SUM=1: the integrating ice kernels sum the normalisation instead of reading its table
    int psd_only = 15;                 // CPOL_PSD_ONLY (tools/psd_flavours.py): bit mask of the flavours to launch (1 gamma-exp, 2 recurrence, 4 ice, 8 melting); results are then incomplete
    long psd_grid = 1024;              // CPOL_PSD_GRID, CPOL_PSD_GRID_GENERIC: persistent grids: 1024 workgroups walk the unit list with a static stride
    long psd_grid_generic = 1024;      // (smaller grids, 512 / 768, measured equal or slower)
    bool psd_siblings = false;         // CPOL_PSD_SIBLINGS=1: the integrating flavours on sibling streams (see choose_forms)
    long psd_lds_pad = 0;              // CPOL_PSD_LDS_PAD: extra dynamic LDS limits the workgroups of k_psd_uniform per CU
    int final_512 = -1;                // CPOL_FINAL_512=0 / 1: never / always k_final with 512 threads (default: by the number of rays)
};

inline const ProcessKnobs &process_knobs()
{
    static const ProcessKnobs pk = [] {
        ProcessKnobs k;
        const auto num = [](const char *name, auto &v) { if (getenv(name)) v = atol(getenv(name)); };
        num("CPOL_GATE1_PRESENT", k.gate1_present);
        num("CPOL_EXP_SKIP", k.exp_skip);
        num("CPOL_LOOKUP_TILE", k.lookup_tile);
        num("CPOL_LOOKUP_FILL", k.lookup_fill);
        num("CPOL_ICE_FORCE_SUM", k.ice_force_sum);
        num("CPOL_PSD_ONLY", k.psd_only);
        num("CPOL_PSD_GRID", k.psd_grid);
        num("CPOL_PSD_GRID_GENERIC", k.psd_grid_generic);
        k.psd_siblings = getenv("CPOL_PSD_SIBLINGS") && atoi(getenv("CPOL_PSD_SIBLINGS")) != 0;
        num("CPOL_PSD_LDS_PAD", k.psd_lds_pad);
        num("CPOL_FINAL_512", k.final_512);
        return k;
    }();
    return pk;
}

// ---- what the rules read ----
struct FormSpecies {                   // of a hydrometeor slot: its integral table (ItabDev) and descriptor (cpol_hydro_desc)
    bool tab = false, two_d = false, writes_vn = false;
    int pan_lo = 0, pan_hi = 0, n_pan = 0;
    int psd_family = 0, numeric_intv = 0, q_source = 0, uniform_grid = 0, tab_degree = 0, rule = 0, var_q = -1;
    bool pre = false, dnu = false;     // per-bin factors staged
};

struct FormIn {
    int n_rays = 0, n_gates = 0, n_sub = 0, n_h = 0, geo_rays = 0;
    bool columns = false, sub_export = false, members = false, timed = false;      // the entry point
    bool melt_given = false, ml = false, skip_melting = false;
    int geometry_mode = 0, doppler = 0;
    bool site = false, versioned = false, with_melting = false, exact_sub = false;
    bool want_latlon = false, want_sz_total = false, want_model = false, reuse = false;
    int outputs_on_device = 0;
    bool keep_debug = false;
    int timing = 0, lanes = 0, nz = 0;
    int scan_form = 0;                 // CPOL_SCAN_FORM of the build (reported, decides nothing)
    bool shadow = false;               // cpol_sweep_params.terrain_shadow: k_terrain_shadow between the interpolation and the classification
    bool want_species = false;         // cpol_outputs.species: the per-species rows sz_integ are kept for k_species
    int n_hydro = 0;
    FormSpecies s[CPOL_MAX_HYDRO];
};

enum { SUM_GATHER = 0, SUM_SMALL, SUM_LDS, SUM_SCALAR, SUM_TEAM };

// ---- what they decide ----
struct Forms {
    int lanes = 0;
    bool ray_prep = false, prep_paths = false, geo_poly = false, poly_single = false;
    bool traj_launch = false, traj_paths = false;      // k_trajectory ahead of the sweep kernel, writing the ray paths
    int melt_qr = -1, melt_qs = -1, melt_qg = -1;      // the 1-moment rain / snow / graupel variables of the melting scheme
    bool sub_melt = false;
    bool any_2d = false, all_tab = false, any_tab = false;
    bool subsum = false, final_inplace = false;
    bool gate1 = false, fused_gate1 = false, by_species = false, gate1_ray = false;
    int g1r = 0;
    bool present = false;                              // k_interp_sweep writes k_gate1_ray's presence words
    int vsrc[CPOL_MAX_HYDRO] = {};                     // FinalArgs::vsrc
    bool any_vsrc2 = false;
    bool rare_direct = false, fused = false, plain_interp = false, stencil = false, drop_latlon = false;
    bool want_szt = false;
    long n_tiles = 0;                                  // ray x gate tiles of k_psd_lookup
    bool use_tile_list = false, lookup_launch = false, lookup_tile = false, rare_fork = false;
    int lookup_split = 1;
    bool psd_need[4] = {false, false, false, false};   // the integrating flavours launched one by one (FORMS_MODE_*)
    bool psd_rare_one = false, psd_fork = false, psd_ice_tab = false, psd_melt_tab = false, psd_melt_direct = false;
    int psd_modes = 0;                                 // k_psd_rare's `modes`
    int sum_form = SUM_GATHER, sum_team = 0, sum_tile_log2 = 0;
    bool sum_chain = false;
    bool rvel_terms = false, final_512 = false, graphable = false;
};

inline Forms choose_forms(const FormIn &in, const Knobs &k, const ProcessKnobs &pk)
{
    Forms f;
    const int n_rays = in.n_rays, ng = in.n_gates, n_sub = in.n_sub, n_hyd = in.n_hydro, mode = in.geometry_mode;
    const long n_rg = (long)n_rays * ng;
    const bool cols = in.columns, sub_out = in.sub_export, mem = in.members, dbg = in.keep_debug;
    const bool doppler = in.doppler != 0, dop2 = in.doppler == 2, dop3 = in.doppler == 3;
    const auto cdiv = [](long a, long b) { return (a + b - 1) / b; };
    f.lanes = in.lanes;
    // several sub-beams: the ray paths (shared by the horizontal nodes of a vertical node) and the per-ray
    // constants of the geodesic come from k_trajectory instead of once per sub-beam gate
    f.ray_prep = n_sub >= FORMS_RAY_PREP_MIN_SUB && !cols;
    f.prep_paths = f.ray_prep && in.n_h > 1 && mode != CPOL_GEOM_HOST_PATHS;
    // ... and ahead of the sweep kernel for the parity access to the paths (cpol_debug_read "traj")
    f.traj_launch = f.ray_prep || (dbg && mode != CPOL_GEOM_HOST_PATHS && !cols);
    f.traj_paths = mode != CPOL_GEOM_HOST_PATHS && (f.prep_paths || dbg);
    // the rotated coordinates of the non-central sub-beams as polynomials of the arc distance (cpol_interp.inl: k_trajectory):
    // ground radars on the 4/3-earth ray paths, one site (CPOL_GEO_POLY=0: the short closed form of round 4)
    f.geo_poly = f.ray_prep && k.geo_poly && mode == CPOL_GEOM_GROUND_43 && !in.site;
    // single-beam sweeps (round 5): the one sub-beam takes the polynomials too when its float64 latitude / longitude are not
    // outputs; they belong to the resident table set of the rays and are made once per (version, range grid)
    // (round 6: also when the float64 latitude / longitude are outputs -- the long form then runs for those two arrays alone and
    // the float32 grid coordinates still come from the guarded polynomials: identical calls give identical bits whether or not the
    // caller fetches the gate coordinates, round-5 advisor finding)
    f.poly_single = !f.ray_prep && !cols && k.geo_poly && k.geo_poly_central && mode == CPOL_GEOM_GROUND_43 && !in.site &&
                    (!dbg || k.geo_poly_central == 2) && in.versioned && !in.exact_sub;
    f.drop_latlon = f.poly_single && !dbg && !in.want_latlon;      // (nobody reads the library's own float64 copies)
    f.all_tab = true;
    for (int j = 0; j < n_hyd; ++j) {
        const FormSpecies &s = in.s[j];
        f.any_tab = f.any_tab || s.tab;
        f.all_tab = f.all_tab && s.tab;
        f.any_2d = f.any_2d || (s.tab && s.two_d);
        if (s.q_source != CPOL_Q_MODEL) continue;
        if (s.rule == CPOL_RULE_RAIN_1MOM) f.melt_qr = s.var_q;
        if (s.rule == CPOL_RULE_SNOW_1MOM) f.melt_qs = s.var_q;
        if (s.rule == CPOL_RULE_GRAUPEL_1MOM) f.melt_qg = s.var_q;
    }
    f.sub_melt = sub_out && in.with_melting && !in.skip_melting;
    // the sub-beam sums by one thread per (gate, hydrometeor) with the 1-D table items evaluated in
    // place (k_subbeam_sum); CPOL_SUBSUM=0: k_psd_lookup stores them and k_final walks the rows
    // (not with Doppler scheme 3: k_spec_atten reads every item's columns from res[]; with one
    // sub-beam there is nothing to accumulate and the extra launch costs more than it saves)
    bool any1d = false;
    for (int j = 0; j < n_hyd; ++j) any1d = any1d || (in.s[j].tab && !in.s[j].two_d);
    const bool subsum_any = k.subsum != 0 && any1d && !dop3;
    // ... with fewer than 4 sub-beams k_final itself evaluates them in place (no extra launch, and
    // k_psd_lookup no longer writes 96 B per item for k_final to read back)
    // -- where that saves the k_psd_lookup launch altogether (no melting species, no Doppler sums from the tables: the
    // C2 sweep 122 -> 119 us and 46 MB less traffic).  Where k_psd_lookup runs anyway it keeps storing the columns: the
    // gathers inside the per-ray workgroups of k_final cost more than the stored rows (C3 sweep at 3 deg: 199 against
    // 188 us; 512-thread workgroups held to 128 / 168 VGPRs: 138 / 159 us on the C2 sweep; round 4)
    f.final_inplace = subsum_any && n_sub < 4;
    for (int j = 0; j < n_hyd && f.final_inplace; ++j)
        if (in.s[j].tab && (in.s[j].two_d || (doppler && in.s[j].writes_vn))) f.final_inplace = false;
    f.subsum = subsum_any && n_sub >= 4;
    // The single-beam fast path (cpol_gate.inl): one sub-beam per radial and every slot on an integral table --
    // k_gate1 takes a gate from its interpolated model values to its polarimetric variables in one kernel
    // (k_classify + k_psd_lookup + the per-gate half of k_final), items outside the tables go to the integrating
    // kernels as one-item work units without the counting sort.  CPOL_GATE1=0 (or CPOL_SUBSUM=0, debug reads, a
    // slot without a table, Doppler scheme 3) keeps the general launch sequence; the results are bit-identical.
    // Not with melting species: their 2-D blocks are walked by whole wavefronts, which inside this one fat kernel
    // (six species in sequence per thread) is no faster than k_classify + k_psd_lookup, and the four idle
    // launches of the integrating flavours cost more than the two bucket launches they replace (C3 sweep at
    // 3 deg: 203 us this way against 188; the kernel handles them -- CPOL_GATE1=2 forces it, tests do).
    // (columns with given melting fields: k_classify's GIVEN form; the single-beam kernels diagnose melting themselves)
    // (hydrometeor contributions, FormIn::want_species: the single-beam kernels keep an absent species as 0.f in registers and never
    // form the NaN-marked rows sz_integ[gate][species][12] that k_species reads; final_gate (k_final) and k_subbeam_sum do.  Such a
    // call takes the general sequence, exactly what CPOL_GATE1=0 gives: no gate1, and with it no gate1_species, gate1_ray or
    // fused_gate1, which all hang on it.  Every other rule is untouched.)
    f.gate1 = k.gate1 != 0 && k.subsum != 0 && n_sub == 1 && !dbg && !dop3 && !in.ml && !in.melt_given && !sub_out &&
              f.all_tab && (k.gate1 == 2 || !f.any_2d) && !in.want_species;
    if (f.gate1) f.final_inplace = true;       // (k_final's recomputed gates take the table items from their records)
    // k_interp_gate1 (CPOL_FUSE_GATE1=1, not the default): the single-beam kernel interpolates its gates too.  Measured: the
    // isolated C2 sweep 95.4 -> 88.6 us (one lane back to back: 70 -> 62 us per sweep), but with three lanes in flight 42.2 ->
    // 44.8 us per sweep, and the Ku swath of config 5 (9 800 rays) 0.93 -> 1.18 ms: at the 3 wavefronts per SIMD k_gate1 needs,
    // the interpolation -- VALU-bound at 5 -- loses more than the saved launch and the 14 MB of vals[] give back.
    // (terrain shadowing: a gate's values depend on the gates in front of it on its sub-beam, which a kernel that interpolates and
    // goes on in one launch has not seen -- the interpolation stays a launch of its own, k_terrain_shadow follows it)
    f.fused_gate1 = k.fuse_gate1 != 0 && f.gate1 && !cols && !mem && !in.shadow;
    // which species' fall-speed sums k_final reads -- 1: vn[] per gate, written by the PSD stage (scheme 2, melting species) or,
    // for the analytic moments of the gamma species under scheme 1, by k_classify; 2: summed over the ray (1-moment ice, numeric
    // integrate_V) and credited to the first valid gate (k_ice_first)
    for (int j = 0; j < n_hyd && doppler && !dop3; ++j) {
        const FormSpecies &s = in.s[j];
        f.vsrc[j] = (dop2 || s.psd_family == CPOL_PSD_MELTING) ? 1 : (s.psd_family == CPOL_PSD_ICE_FIELD || s.numeric_intv) ? 2 : 1;
        f.any_vsrc2 = f.any_vsrc2 || f.vsrc[j] == 2;
    }
    // one wavefront per species (k_gate1_species) where no melting species and no per-ray fall-speed sums are involved
    // -- for small launches: the C2 sweep (8 wavefronts per SIMD) 33.6 -> 30.7 us and 42.9 -> 39.2 us per sweep with three
    // lanes in flight; the C5 Ku swath (235 per SIMD, five species) 429 -> 674 us: every species' wavefront repeats the
    // gate's loads and wavefronts 1.. idle while wavefront 0 finishes the gates; five C2 sweeps as one sequence (44 per
    // SIMD) 112 -> 100 us (CPOL_GATE1_SPECIES=0 / 2: never / always)
    const long g1_waves_per_simd = n_rg * n_hyd / 64 / 1024;
    f.by_species = f.gate1 && (k.gate1_species == 2 || (k.gate1_species == 1 && g1_waves_per_simd < 48)) &&
                   !f.fused_gate1 && !f.any_2d && !f.any_vsrc2 && !in.with_melting;
    // k_gate1_ray (cpol_gate.inl): the single-beam kernel with one wavefront per species, the ray's range scans by the
    // workgroup that finishes the ray last and the items outside the tables integrated in place -- the sweep is
    // k_interp_sweep + that kernel, no integrating launch, no k_final.  Only where the in-place integration mirrors the
    // integrating kernels: gamma-family species without Doppler-scheme-2 sums and without per-ray fall-speed totals
    // (numeric_intv), whose tables kept all panels but the tail (an item off the table costs a wavefront ~40 us:
    // fine for the handful a volume has, not for a table that lost half of its panels to the accuracy gate).
    f.g1r = k.gate1_ray >= 0 ? k.gate1_ray : (in.lanes >= 2 ? 1 : 0);
    f.gate1_ray = f.by_species && f.g1r && !k.fuse_gate1 && !dop2 && n_rays <= 65535;
    for (int j = 0; j < n_hyd && f.gate1_ray; ++j) {
        const FormSpecies &s = in.s[j];
        f.gate1_ray = s.psd_family == CPOL_PSD_GAMMA && !s.numeric_intv && s.q_source == CPOL_Q_MODEL && s.tab && !s.two_d &&
                      ((s.pan_lo == 0 && s.pan_hi >= s.n_pan - 2) || f.g1r >= 2) && s.pre && s.dnu;
    }
    // (columns, members: no presence words are written; terrain shadowing: they would be written from unshadowed values)
    f.present = f.gate1_ray && pk.gate1_present && !cols && !mem && !in.shadow;
    // Every slot on an integral table: the items outside the tables (a handful per volume) are listed directly as
    // one-item work units by k_classify / k_gate1 -- key in b_pos, gate in b_perm, count in b_totals -- and the
    // counting sort (LDS ranking in k_classify, k_bucket_scan, k_bucket_scatter) is not run at all.  CPOL_RARE_DIRECT=0,
    // debug reads (bucket counts) or a slot without a table keep the sort: with EVERY item integrated one item per
    // work unit would waste 63 of 64 lanes.
    // (Measured and dropped: the sort's chain -- scan, scatter, the integrating kernels, all idle when every item lies
    // on a table -- on a sibling stream beside k_psd_lookup, forked and joined with events: the isolated C2 sweep
    // 122 -> 135 us, the C3 volume 468 -> 476 us, the 225-ray C4 share 1.568 -> 1.553 ms: a cross-stream event
    // costs the device about as much as the three idle launches it would hide.)
    f.rare_direct = (f.gate1 || (k.rare_direct != 0 && !dbg)) && f.all_tab;
    f.want_szt = in.want_sz_total || dbg;
    // every slot on a table, no debug reads: the gate kernel classifies its gates itself (k_interp_classify, cpol_fused.inl)
    // (never for columns: the forms that interpolate, k_interp_classify and k_interp_gate1, are replaced by k_columns_ingest)
    // (nor with terrain shadowing: see fused_gate1 above -- the path CPOL_FUSE_CLASSIFY=0 takes)
    f.fused = k.fuse_classify != 0 && f.rare_direct && !f.gate1 && !in.ml && !dop3 && !dbg && !cols && !sub_out && !mem && !in.shadow;
    f.plain_interp = !cols && !mem && !f.fused && !f.fused_gate1 && !(pk.exp_skip & 1);
    // A launch that is plain k_interp_sweep, of a single beam whose float32 grid coordinates alone are wanted, under a caller's
    // version tag: the gate stencil of its (geometry, heights) pair -- noted at first sight, recorded at the second, replayed from
    // the third on (cpol_interp.inl).  Everything else keeps k_interp_sweep.
    f.stencil = f.plain_interp && n_sub == 1 && !sub_out && mode != CPOL_GEOM_HOST_PATHS && !f.prep_paths && f.drop_latlon &&
                in.versioned && !k.use_graph && in.nz < 32768;
    // k_psd_lookup's workgroups first list the tiles among their own that hold a species with a 2-D table (LookupArgs::tile_scan):
    // when the lookup walks tiles and has nothing but the 2-D tables to evaluate, from 262 144 tiles on (C4 volume, 735 000 tiles:
    // 1.30 -> 1.20 ms; its share of 1/8, 92 000 tiles: 247 -> 239-257 us, nothing gained.  Measured and dropped on the way: the
    // list in global memory, made by k_interp_classify with one bit per tile and an atomicOr per item -- lookup 1.30 -> 1.09 ms
    // and 239 -> 205 us, but the classification 3.24 -> 4.31 ms: device-scope atomics; made by a kernel of its own with one
    // atomicAdd per wavefront and pass -- the same lookup times, and 244 / 51 us for that kernel: one address, ~11 ns per atomic)
    constexpr int TILE_GATES = 1 << FORMS_TILE_GATES_LOG2, TILE_RAYS = 64 >> FORMS_TILE_GATES_LOG2;
    f.n_tiles = cdiv(n_rays, TILE_RAYS) * n_sub * cdiv(ng, TILE_GATES);
    const bool inplace = f.subsum || f.final_inplace;
    if (k.lookup_list && f.rare_direct && !f.gate1 && pk.lookup_tile && n_rays >= TILE_RAYS && inplace &&
        (f.n_tiles >= 262144 || k.lookup_list == 2) && f.n_tiles < (1L << 31)) {
        bool other = false;
        for (int j = 0; j < n_hyd; ++j) {
            const FormSpecies &s = in.s[j];
            if (s.tab && !s.two_d && ((dop3 && s.psd_family == CPOL_PSD_ICE_FIELD) || (f.final_inplace && doppler && s.writes_vn))) other = true;
        }
        f.use_tile_list = f.any_2d && !other;
    }
    // items on an integral table (k_psd_lookup) -- with k_subbeam_sum / in-place evaluation in k_final: only for 2-D tables,
    // Doppler sums and the ice intercept (k_subbeam_sum evaluates the Doppler sums itself)
    bool lookup = f.any_tab && !inplace;
    for (int j = 0; j < n_hyd && f.any_tab && !lookup; ++j) {
        const FormSpecies &s = in.s[j];
        if (s.tab) lookup = s.two_d || (dop3 && s.psd_family == CPOL_PSD_ICE_FIELD) || (f.final_inplace && doppler && s.writes_vn);
    }
    f.lookup_launch = lookup && !f.gate1;
    f.lookup_tile = f.any_2d && pk.lookup_tile && n_rays >= TILE_RAYS;
    // few wavefronts (a single sweep with one sub-beam): the walk of the busiest tile is the kernel's duration;
    // its distinct blocks and species are dealt to `split` wavefronts (CPOL_LOOKUP_SPLIT=<n>; default by launch size)
    const long lookup_waves_per_simd = (f.lookup_tile ? f.n_tiles * 64 : n_rg * n_sub) / 64 / 1024;
    f.lookup_split = k.lookup_split > 0 ? k.lookup_split : (f.lookup_tile && lookup_waves_per_simd < 16) ? 4 : 1;
    // the items outside the tables (k_psd_rare) and the 2-D table items (k_psd_lookup) are disjoint and both wait for
    // the classification alone: k_psd_rare goes to a sibling stream that forks in front of k_psd_lookup and joins before the
    // sub-beam sums -- its one busy workgroup (69-80 us for a single item of the C4 volume) runs beside the lookup
    f.rare_fork = f.lookup_launch && k.rare_overlap && f.rare_direct && k.psd_rare && !k.use_graph && !dbg;
    // PSD x scattering table: one launch per kernel flavour present ...
    for (int j = 0; j < n_hyd; ++j) {
        const FormSpecies &s = in.s[j];
        const int m = s.psd_family == CPOL_PSD_ICE_FIELD ? FORMS_MODE_ICE : s.psd_family == CPOL_PSD_MELTING ? FORMS_MODE_MELTING
                    : s.uniform_grid ? FORMS_MODE_GAMMA_UNIFORM : FORMS_MODE_GAMMA_EXP;
        if (pk.psd_only & (1 << m)) f.psd_need[m] = true;
        // slots with lambda tables: k_psd_ice2 takes the units inside the tabulated range (all of them, in practice), k_psd<ICE>
        // sums the others; melting slots with fw tables go to the table-driven kernel, the others (none in the product's own
        // staging) to the direct one; each skips foreign units
        if (s.psd_family == CPOL_PSD_ICE_FIELD && s.uniform_grid && s.tab_degree == CPOL_ICE_DEGREE) f.psd_ice_tab = true;
        if (s.psd_family == CPOL_PSD_MELTING) (s.tab_degree == CPOL_MELT_DEGREE ? f.psd_melt_tab : f.psd_melt_direct) = true;
    }
    // ... items listed directly (every slot on a table): ONE launch runs every flavour (k_psd_rare); CPOL_PSD_RARE=0: a launch
    // per flavour as before (same bits: tests/test_gpu_edges.py)
    f.psd_rare_one = f.rare_direct && k.psd_rare && pk.psd_only == 15 && !pk.psd_siblings && !dbg;
    if (f.psd_rare_one) {
        for (int m = 0; m < 4; ++m) { if (f.psd_need[m]) f.psd_modes |= 1 << m; f.psd_need[m] = false; }
        if (f.psd_melt_direct) f.psd_modes |= 16;
    }
    // The flavours touch disjoint items and could run side by side.  Measured (MI355X, one
    // sweep): on sibling streams (fork after the bucket sort, join before the final stage) the
    // PSD stage took 762 vs 734 us on C3 and 29.2 vs 27.1 ms on C4 -- every flavour is a
    // persistent grid that fills the chip and is VALU-bound, so overlap only adds the event
    // traffic.  Back to back on the sweep's stream is the default; CPOL_PSD_SIBLINGS=1 forks.
    f.psd_fork = pk.psd_siblings && f.psd_need[0] + f.psd_need[1] + f.psd_need[2] + f.psd_need[3] > 1;
    if (f.subsum) {
        // lanes of a wavefront = a tile of neighbouring rays x consecutive gates (16 x 4 from 16 rays on)
        int tl = FORMS_TILE_GATES_LOG2;
        while (tl < 6 && (64 >> tl) > n_rays) ++tl;
        f.sum_tile_log2 = tl;
        // the scalar-cache form needs many wavefronts per SIMD to hide its waits (C4 volume, rays per sweep:
        // 45 / 90 / 180 / 360 -> PSD stage 1.08 / 1.56 / 2.08 / 3.57 ms against 0.85 / 1.48 / 2.35 / 4.71 ms with
        // the gather): from ~32 wavefronts per SIMD on (the scalar-cache form; see below for the LDS form).  CPOL_SUBSUM_COOP=0 / 1: never / always.
        // With lanes (cpol_fork) other sweeps share the GPU and hide the waits: measured with three lanes in
        // flight, the share of one of 8 / 4 GPUs (11 / 21 wavefronts per SIMD): 1.30 / 2.24 ms per volume share
        // against 1.31 / ~2.5 ms with the gather -- from ~12 there.
        // (round 4, with the validity bits read up front: the share of one of 8 GPUs -- 11 wavefronts per SIMD --
        // with three lanes in flight 1.19 ms per volume share this way against 1.27 with the gather: from 8 there)
        // (the LDS form, round 4: the share of one of 8 / 4 / 2 GPUs alone -- 11 / 21 / 43 wavefronts per SIMD -- PSD stage 905 / 1281 /
        // 1748 us against 846 / 1413 / 2312 with the gather: from 16 there)
        const long waves_per_simd = cdiv(n_rays, 64 >> tl) * cdiv(ng, 1 << tl) * n_hyd / 1024;
        const bool coop = k.subsum_coop == 1 || (k.subsum_coop < 0 && waves_per_simd >= (in.lanes >= 2 ? 8 : 16));
        // the team form (round 5: W wavefronts per (tile, species) share the sub-beams, the float32 sums stay ordered): what bounds a small
        // launch is the length of its longest wavefront's chain (cpol_final.inl).  Share of one of 8 / 4 / 2 GPUs alone (11 / 21 / 43
        // wavefronts per SIMD), ms per volume share: 1.47 / 2.18 / 3.57 with the rule above, 1.23 / 2.00 / 3.53 with W = 2 (W = 4: 1.23 /
        // 2.05 / 3.66; W = 4 with the sums handed on in LDS instead of a barrier per round -- the default -- 1.16 / 1.98 / 3.44); with three lanes in flight 0.97 / 1.71 either way (a context WITH lanes that runs one share at
        // a time: 1.42 with the LDS form its rule picked, 1.23 with the team); the whole volume 1.71 (LDS form) against 1.94 ms.
        const int team = k.subsum_team >= 0 ? k.subsum_team       // (a form forced through CPOL_SUBSUM_COOP stays what was asked for)
                       : (k.subsum_coop < 0 && waves_per_simd < 50 ? 4 : 0);      // (whatever the lanes: a context with lanes may still run one sweep at a time)
        // the cooperative form: coefficient rows through LDS (default since round 4) or through the scalar cache (CPOL_SUBSUM_FORM=scalar).
        // CPOL_SUBSUM_SMALL=1 (experiment, never the default): the gather form with three wavefronts per (tile,
        // hydrometeor), 4 columns each, and all rows of the block requested at once -- see the note on SPLIT in
        // cpol_final.inl: slower than the plain gather on the share (571 vs 533 us) and with lanes (1.41 vs 1.27 ms)
        f.sum_form = (team >= 2 && team <= 8) ? SUM_TEAM : (coop && k.subsum_scalar) ? SUM_SCALAR : coop ? SUM_LDS
                   : k.subsum_small == 1 ? SUM_SMALL : SUM_GATHER;
        f.sum_team = f.sum_form == SUM_TEAM ? team : 0;
        f.sum_chain = k.subsum_chain != 0 || team == 8;            // (W = 8 exists in the chained form alone)
    }
    // the per-sub-beam velocity terms by one thread per sub-beam gate (k_rvel_terms; k_final adds them in order)
    f.rvel_terms = doppler && !dop3 && n_sub >= 4;
    // (k_final, one workgroup per ray: with no more rays than CUs the kernel lasts as long as ONE workgroup -- 512
    // threads halve its gate loop; the share of one of 8 GPUs of a 5 x 360-ray volume is 225 rays)
    f.final_512 = (pk.final_512 == 1 || (pk.final_512 < 0 && n_rays <= 256)) && ng > FORMS_FINAL_THREADS;
    // The launch sequence as a HIP graph (CPOL_USE_GRAPH=1): with device outputs and nothing to upload it is captured and
    // replayed while the arguments stay the same (one graph launch instead of ten kernel launches).
    f.graphable = k.use_graph && in.outputs_on_device == 1 && in.timing == 0 && !dbg && mode != CPOL_GEOM_HOST_PATHS && !cols && !sub_out &&
                  !mem && !dop3 && in.reuse && !f.want_szt && !in.want_model && !in.shadow && !in.want_species;
    return f;
}

// cpol_debug_read "launch_forms" (Context.FORM_NAMES in _native.py), also mixed into the graph key; [11], graph replayed, is set after the launch
inline void forms_record(const FormIn &in, const Forms &f, int out[12])
{
    const int v[12] = {f.g1r, (int)f.gate1_ray, (int)f.gate1, (int)f.fused, (int)f.rare_direct, (int)f.subsum, (int)f.final_inplace,
                       (int)f.poly_single, in.n_sub, in.lanes, in.scan_form, 0};
    memcpy(out, v, sizeof v);
}
