// cosmo_pol_hip.hip -- C ABI (include/cosmo_pol_amd.h) and launch sequence of
// the MI355X-native cosmo_pol hot path.  gfx950 only; no CPU fallback.
//
// One call of cpol_run_sweep = the work of one `pool.map(worker, azimuths)`
// of the reference (cosmo_pol/radar_operator.py:429-432) for the rays given:
//
//   k_interp_sweep    (ray, sub-beam, gate)           ray path (4/3 earth / orbit), geodesic,
//                                                     rotated pole, trilinear gather, all vars
//   k_classify        (sub-beam gate)                 melting, PSD parameters,
//                                                     LUT bins, bucket histogram
//   k_bucket_scan / k_bucket_scatter                  counting sort by LUT slice + unit list
//   k_psd_{uniform,gamma,ice,melting}                 PSD x table integration
//   k_final           (ray)                           sub-beam/hydrometeor sums, polarimetric
//                                                     variables, range scans, sensitivity
// = 6 launches for a 1-moment sweep (10 before the ray-path, unit-list and final merges).
#include <hip/hip_runtime.h>
#include <math.h>
#include <mutex>
#include <stdio.h>
#include <time.h>
#include <string.h>
#include <string>
#include <type_traits>
#include <vector>

#include "cpol_device.h"
#include "cpol_tile.h"
#include "cpol_forms.h"
#include "cpol_place.h"
#include "cpol_buffers.h"
#include "cpol_hist.h"
#include "cpol_comp.h"
#include "cpol_frac.h"
#include "cpol_obj.h"
#include "cpol_products.h"
#include "cpol_interp.inl"
#include "cpol_psd.inl"
#include "cpol_fused.inl"
#include "cpol_final.inl"
#include "cpol_gate_ops.h"
#include "cpol_gate.inl"
#include "cpol_spectrum.inl"
#include "cpol_ingest.inl"
#include "cpol_superob.inl"
#include "cpol_member_stats.inl"
#include "cpol_hist.inl"
#include "cpol_comp.inl"
#include "cpol_frac.inl"
#include "cpol_frac_prob.inl"
#include "cpol_obj.inl"
#include "cpol_shadow.inl"
#include "cpol_species.inl"

static_assert(FORMS_RAY_PREP_MIN_SUB == CPOL_RAY_PREP_MIN_SUB && FORMS_TILE_GATES_LOG2 == CPOL_TILE_GATES_LOG2 &&
              FORMS_FINAL_THREADS == CPOL_FINAL_THREADS && (int)FORMS_MODE_GAMMA_EXP == (int)PSD_MODE_GAMMA_EXP &&
              (int)FORMS_MODE_GAMMA_UNIFORM == (int)PSD_MODE_GAMMA_UNIFORM && (int)FORMS_MODE_ICE == (int)PSD_MODE_ICE &&
              (int)FORMS_MODE_MELTING == (int)PSD_MODE_MELTING, "cpol_forms.h: the build constants of the kernel files");
static_assert(BUF_GEO_NP == CPOL_GEO_NP && BUF_MAX_PAR == CPOL_MAX_PAR && BUF_COUNT_SLOTS == CPOL_COUNT_SLOTS &&
              BUF_ICEFIRST_BYTES == sizeof(IceFirst) && BUF_WORKUNIT_BYTES == sizeof(WorkUnit), "cpol_buffers.h: the build constants of the kernel files");

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

enum { EV_T0 = 0, EV_TRAJ, EV_INTERP, EV_CLASSIFY, EV_BUCKET, EV_PSD, EV_FINAL, EV_N };

// scattering table kept resident for a caller-supplied cpol_hydro_desc.table_id
struct TableCacheEntry {
    uint64_t id = 0;
    size_t bytes = 0;
    DevBuf buf;
    uint64_t used = 0;
};

// integral tables kept for a caller-supplied cpol_hydro_desc.table_id
struct ItabCacheEntry {
    uint64_t id = 0;
    int dop2 = 0;
    DevBuf tab, head;
    ItabDev t{};
    double check = 0.0, check_at = 0.0, check_edge = 0.0;
    uint64_t used = 0;          // build serial of the last use (LRU; entries of the current build are pinned)
};

// ---- gate stencils (cpol_interp.inl: k_interp_record / k_interp_replay) ----
// Everything interp_gate reads before gate_value, compared bytewise (zeroed before it is filled: no stray padding)
struct StencilKey {
    uint64_t version, heights;  // the caller's table version; the root's heights identity
    long shape[6];              // of the table set
    double range0, range_step, ke, re, alt, lon, sin_u1, cos_u1, poly_scale;
    int mode, poly, exact, pad;
};

struct StencilEntry {
    StencilKey key;
    uint64_t id = 0;
    int state = 0;              // 0 noted (seen once), 1 its recording launch is being queued, 2 recorded
    bool refused = false;       // the record did not fit the budget or the device: the geometry keeps the full form
    void *buf = nullptr;
    size_t bytes = 0;
    long n_pad = 0;             // gates, rounded up to 64
    hipEvent_t ev = nullptr;    // behind the recording launch, on the recorder's stream
};

}  // namespace

struct cpol_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // lanes (cpol_fork): a child shares the parent's staged model / tables read-only and
    // owns only its stream, work buffers and counters
    cpol_ctx *parent = nullptr;
    int n_children = 0;
    // HIP graph of the sweep's launch sequence (device outputs, unchanged arguments)
    Knobs knobs;                       // the launch-rule knobs of the environment (cpol_forms.h), read when the context is created
    hipGraphExec_t graph_exec[2] = {nullptr, nullptr};     // one per counter set (the sets alternate sweep by sweep)
    uint64_t graph_key[2] = {0, 0};
    uint64_t stage_serial = 0;         // bumped by every staging call (kernel arguments change)
    std::string err;
    // model
    bool model_staged = false;
    ModelDev model{};
    DevBuf d_H, d_V;
    // ensemble members (cpol_stage_member): the cubes of members 1, 2, ... -- member 0 is d_V; same shape, grid and level heights
    // (d_H is shared).  Owned by the root context; a lane reads its parent's.  member_sel: whose cube model.V points to
    std::vector<DevBuf> members;
    int member_sel = 0;
    double ingest_ms[4] = {0, 0, 0, 0};   // the last cpol_stage_model_packed (cpol_debug_read "ingest_times")
    // hydrometeors
    HydroSet hs{};
    SpecSet ss{};
    DevBuf d_table[CPOL_MAX_HYDRO], d_pre[CPOL_MAX_HYDRO], d_dnu[CPOL_MAX_HYDRO],
        d_aux[CPOL_MAX_HYDRO], d_rcsw[CPOL_MAX_HYDRO], d_rcs32[CPOL_MAX_HYDRO], d_dgrid[CPOL_MAX_HYDRO];
    bool hydro_staged[CPOL_MAX_HYDRO] = {};
    // integral tables (built on the device by build_itabs after staging; lanes share the parent's)
    DevBuf d_itab[CPOL_MAX_HYDRO], d_itab_head[CPOL_MAX_HYDRO], d_itab_M, d_itab_M1;
    std::vector<ItabCacheEntry> itab_cache;
    std::vector<TableCacheEntry> table_cache;  // staged scattering tables with a table_id
    uint64_t table_clock = 0;
    uint64_t itab_builds = 0;
    double itab_check_at[CPOL_MAX_HYDRO] = {};
    double itab_check[CPOL_MAX_HYDRO] = {};     // worst deviation at the blocks' check points (negative: table rejected)
    std::vector<double> itab_detail[CPOL_MAX_HYDRO];   // 1-D tables: [log2_lo, ppo, d0, n_pan, worst per function (NF), worst per panel (n_pan)]
    double itab_ms[CPOL_MAX_HYDRO][2] = {};     // device time of the last build of the slot's table: all of it, the check alone
    double itab_check_edge[CPOL_MAX_HYDRO] = {};   // 1-D tables: worst deviation at the second check point (near the panel edge) alone
    double itab_bad[CPOL_MAX_HYDRO] = {};       // 1-D tables: (block, function) pairs at or above the accepted deviation
    ItabSet its{};
    uint64_t lut_serial = 0;           // bumped by the staging calls the integral tables depend on (not the model cube)
    uint64_t itab_serial = ~0ull;      // lut_serial the tables were built for
    DevBuf d_tfun[CPOL_N_TFUN];        // host-tabulated float32 functions of T (cpol_stage_t_function)
    const float *tfun[CPOL_N_TFUN] = {};
    // per-sweep work buffers (grow only)
    // per-sweep host tables: packed into ONE pinned staging buffer (ring of 4, an event each) and
    // moved by ONE host-to-device copy into the arena of a table set (tsets[]); v_* = views into the set in use
    // The per-ray tables of the last CPOL_TABLE_SETS scan geometries stay on the device, found again by the
    // caller's version tag: a scan that cycles through its elevations uploads each set once (a 35 KB copy in
    // front of a 0.09 ms sweep costs the stream 25-45 us: measured with tools/submit_cost.py, one lane,
    // 8 elevations in turn: 115 us per sweep against 70 with one resident set).
    struct TableSet {
        uint64_t version = 0, last_use = 0;
        long shape[6] = {0, 0, 0, 0, 0, 0};
        DevBuf buf;
        void *views[11] = {nullptr};
        // single-beam sweeps: the coordinate polynomials of this set's rays (k_trajectory), made once per (version, range grid)
        DevBuf poly;
        uint64_t poly_version = 0;
        double poly_scale = 0.0;
        // ... and per (model grid rotation, radar site): k_trajectory bakes the rotated-pole matrix of the staged model and
        // the site's constants into them (cpol_stage_model clears poly_version; the site is compared sweep by sweep)
        double poly_site[3] = {0.0, 0.0, 0.0};
    };
    static constexpr int N_TABLE_SETS = 8;
    TableSet tsets[N_TABLE_SETS];
    uint64_t tset_clock = 0;
    void *v_traj_in = nullptr, *v_geo = nullptr, *v_subh = nullptr, *v_subv = nullptr, *v_subw = nullptr,
         *v_sens = nullptr, *v_site = nullptr, *v_nyq = nullptr, *v_subsmooth = nullptr,
         *v_mlfilter = nullptr, *v_varray = nullptr;
    // sibling streams of the PSD stage: the kernel flavours of a sweep (recurrence / full-exp /
    // ice / melting) touch disjoint items, so they run side by side (fork after the bucket
    // sort, join before the final stage) instead of back to back
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    struct Staging { void *p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; } stg[4];
    int stg_next = 0;
    DevBuf b_traj, b_wgate, b_clk, b_rayc, b_poly, d_geoM;
    DevBuf b_beam, b_spectrum, b_outwin, b_superob;
    DevBuf b_smom, b_smcount, b_smvar;     // spectrum moments (cpol_spectrum_moments): the two output arrays; the hook's velocity bins
    DevBuf b_spout[SP_N];                  // hydrometeor contributions (cpol_species): its output arrays outside a window image and the caller's device memory
    // ensemble statistics (cpol_member_stats): the running state of this context's pass, and the block k_member_finish writes
    // when the outputs are host memory outside a window image
    DevBuf b_mstate, b_msout;
    DevBuf b_mstash;                       // ... and the members of the fields with quantiles or a verification: [capacity][n_cells] each, sized when a pass begins
    // sweep histograms (cpol_histogram): the running state of this context's pass (the uint64 counts themselves), the rounded
    // edges of the pass, the counts of a finishing call outside a window image and the caller's device memory; the pass (cpol_hist.h)
    DevBuf b_hstate, b_hedges, b_hcounts[CPOL_HIST_FIELDS];
    HistPass hpass;
    std::vector<char> hedges_host;         // ... and what b_hedges holds (the source of its copy)
    // gridded composites (cpol_composite): the running state of this context's pass (max, min, echo-top and count states), the
    // edges of the pass, the per-ray sines and cosines of the call, the maps of a finishing call outside a window image and the
    // caller's device memory (nine `values`, then `count`); the pass (cpol_comp.h)
    // with height layers: b_ctab holds the float32 layer edges and the column tables (per field with one: the float64 values,
    // then the float32 breakpoints), and b_cout gains nine `column` and nine `column_layers`
    // with the exact sums (CPOL_COMP_SUM): b_cwtab holds the weight tables (per field with one: the float64 values, then the
    // float32 breakpoints), and b_cout gains nine `sum` and nine `sum_skipped`
    DevBuf b_cstate, b_cedges, b_crays, b_cout[5 * CPOL_COMP_FIELDS + 1], b_ctab, b_cwtab;
    // ... and the gate planes (CPOL_COMP_PLANE_GATES with host arrays): gate_x then gate_y of the last N_COMP_PLANES non-zero
    // plane_version tags stay on the device, as the table sets do, so the radars of a network that alternate in one pass do not
    // evict each other; a call without a tag uploads into b_cplane.  cplane_stat: {uploads, hits} (cpol_debug_read "composite_plane")
    struct CompPlane {
        uint64_t version = 0, last_use = 0;
        size_t gates = 0;
        DevBuf buf;
    };
    static constexpr int N_COMP_PLANES = 32;
    static_assert(N_COMP_PLANES >= N_TABLE_SETS, "a gate plane per resident table set");
    CompPlane cplanes[N_COMP_PLANES];
    uint64_t cplane_clock = 0;
    int64_t cplane_stat[2] = {0, 0};
    DevBuf b_cplane;
    CompPass cpass;
    CompPlan cplan;                        // ... and the plan of the call at hand (kept here: a call without the struct constructs none)
    std::vector<double> cedges_host;       // ... and what b_cedges holds (the source of its copy)
    std::vector<double> ctab_host;         // ... and what b_ctab holds
    std::vector<double> cwtab_host;        // ... and what b_cwtab holds
    // neighbourhood verification (cpol_fractions): the summed-area tables, the caller's observation and domain on the device (host
    // outputs), `sums` and `totals` outside a window image and the caller's device memory, the maps of the test hook; the plan of
    // the call at hand; prob_sums, reliability, member_sum and member_any of the neighbourhood ensemble probabilities
    // (cpol_fraction_probabilities) are b_fout[12 ... 15]
    DevBuf b_fsat, b_fobs, b_fout[21], b_fmaps;
    FracPlan fplan;
    // object cells (cpol_objects, beside a cpol_fractions): the labelling scratch and the plan of the call at hand; n_objects, table
    // and labels are b_fout[2 ... 4], volume, skipped, field and field_cells of the exact sums b_fout[5 ... 8]; the sums'
    // accumulators and the weight table lie behind the labelling scratch (ObjPlan); n_pieces, pieces and covered of the match
    // b_fout[9 ... 11], the piece scratch behind everything else; correlation, shift, n_pieces, pieces and covered of the track
    // (cpol_objects_track) b_fout[16 ... 20], the track scratch behind the piece scratch
    DevBuf b_oscr;
    ObjPlan oplan;
    DevBuf b_mvobs;                        // verification (cpol_member_verify) with host outputs: the caller's observations on the device
    struct MemberPass {
        bool open = false;
        long n_cells = 0, folded = 0;
        unsigned fields = 0;
        int min_members = 0;
        int n_thr[CPOL_MS_FIELDS] = {};
        double thr[CPOL_MS_FIELDS][CPOL_MS_MAX_THR] = {};
        MemberState st[CPOL_MS_FIELDS] = {};
        // quantiles: the terms as the caller gave them, and each such field's stash
        int q_capacity = 0, q_method = 0;
        bool q_any = false;
        int n_q[CPOL_MS_FIELDS] = {};
        double q[CPOL_MS_FIELDS][CPOL_MS_MAX_Q] = {};
        void *stash[CPOL_MS_FIELDS] = {};
        // verification (cpol_member_verify): the pass was begun with the struct, and its terms
        bool v_on = false;
        unsigned v_fields = 0;
        int v_fair = 0;
    } mpass;
    size_t spec_lds_allowed = 64 * 1024;   // (root context) the largest dynamic LDS asked for k_spec_gate so far (hipFuncSetAttribute)
    size_t hist_lds_allowed[2][3] = {{64 * 1024, 64 * 1024, 64 * 1024}, {64 * 1024, 64 * 1024, 64 * 1024}};   // (root context) the same per instantiation of k_hist: [T is float64][the ordinate's type]
    DevBuf b_bsigma, b_bon;                // spectrum broadening: sigma in bins per sub-beam gate, switch per (ray, sub-beam)
    DevBuf b_vals, b_mask, b_elev, b_coords, b_qmelt, b_fwmelt, b_key, b_par, b_count, b_offset,
        b_units, b_totals, b_perm, b_res, b_pos, b_vn, b_icefirst, b_rvel, b_proj, b_blkranked, b_rec, b_vmask, b_gscan, b_defer;
    DevBuf b_out[16], b_szinteg, b_sztotal, b_model, b_ticket, b_mask8, b_vis;
    DevBuf b_present;                  // k_gate1_ray's sweeps: one word per (ray, 64-gate tile), which hydrometeor slots may have an item there (k_interp_sweep writes, k_gate1_ray reads)
    DevBuf b_colin;                    // cpol_run_columns with host inputs: the caller's columns on the device, read by k_columns_ingest
    DevBuf b_xscr, b_xgeo;             // cpol_interp_subbeams: the long-form gate kernel's scratch values, the geometry of every sub-beam
    DevBuf b_timed;                    // a time-blended sweep: [n_rays] state indices, then [n_rays] weights (k_interp_timed reads them)
    std::vector<char> timed_shadow;    // ... and what b_timed holds (host copy): unchanged brackets are not uploaded again
    // last sweep shapes (debug reads)
    long last_n_sbg = 0, last_n_rg = 0;
    int last_n_rays = 0, last_n_gates = 0, last_n_sub = 0, last_n_v = 0, last_n_keys = 0;
    // Two sets of sweep counters (b_count, b_totals), used in turn: the first kernel of a launch sequence clears
    // the set of the NEXT sweep, so that a kernel which counts can also be the first of its sequence (a kernel cannot
    // clear what its own workgroups add to), and no sequence needs a fill kernel.  Both sets are zero when (re)allocated.
    uint64_t sweep_serial = 0;
    long count_stride = 0;             // ints per set of b_count
    bool counters_dirty = false;       // a launch sequence began and did not end in sweep_serial advancing (an error return after
                                       // its first launch): both counter sets are cleared before the next sequence uses one
    int last_par = 0;                  // the set the last sweep used
    uint64_t graph_captures = 0;       // launch sequences captured into a HIP graph so far (cpol_debug_read "graph_captures": a test hook)
    int last_forms[12] = {0};          // the launch forms of the last sweep (cpol_debug_read "launch_forms"): [0] g1r, [1] k_gate1_ray, [2] single-beam gate kernel,
                                       // [3] k_interp_classify, [4] items off the tables listed directly, [5] k_subbeam_sum, [6] table items evaluated in place,
                                       // [7] coordinate polynomials for the one sub-beam, [8] n_sub, [9] lanes alive, [10] CPOL_SCAN_FORM (1: the range scans by a whole wavefront), [11] HIP graph replayed
    // Gate stencils.  The store lives on the ROOT context (lanes die at every model load; they reach it through `parent`), its
    // bookkeeping under st_mu.  No entry is freed while lanes exist or sweeps are in flight: entries die in cpol_destroy, when the
    // heights identity changes (cpol_stage_model*, which refuse to run while lanes exist and drain the stream) and when the budget is
    // lowered below what is held ("stencil_budget", refused while lanes exist).
    std::mutex st_mu;
    std::vector<StencilEntry *> st_entries;
    size_t st_budget = (size_t)1 << 30, st_bytes = 0;
    uint64_t st_heights = 1;           // heights identity: H, HT, nz / ny / nx, llc / urc / res, the rotation constants
    uint64_t st_next_id = 1, st_records = 0, st_replays = 0, st_drops = 0;
    double model_pole[2] = {0.0, 0.0};
    DevBuf d_hdiff;                    // k_stage_heights_cmp's flag
    // ... and per context (lane): the form of its last sweep (0 full, 1 recording, 2 replay), the entries whose recording launch its
    // stream is known to run behind (one hipStreamWaitEvent per (lane, entry))
    int last_stencil = 0;
    std::vector<uint64_t> st_seen;
    int last_poly_central = 0;         // the last sweep's one sub-beam took the coordinate polynomials (cpol_debug_read "poly_central")
    const void *last_poly = nullptr;   // the coefficient array the last sweep's gate kernel read (b_poly or its table set's), [last_poly_fits][2][CPOL_GEO_NP]
    long last_poly_fits = 0;           // (cpol_debug_read "geo_poly": a test hook)
    bool last_subsum = false;          // the 1-D table items of the last sweep never went through res[] (k_subbeam_sum)
    bool last_vmask = false;           // the last sweep left vmask[] of every sub-beam gate (the general launch sequence)
    bool last_vn = false;              // ... and vn[] of every valid item (Doppler scheme 1)
    bool last_icefirst = false;        // ... and k_ice_first ran (a species whose fall-speed sums are totals over the ray)
    bool keep_debug = false;
    // host time of cpol_run_sweep by section (ns, summed; cpol_debug_read "host_times"): [0] calls, [1] per-ray tables
    // (staging memcpy + the H2D copy call), [2] work-buffer checks / allocations, [3] kernel launches, [4] the
    // device-to-host copy call(s), [5] everything
    // [6..9]: section [1] split: waiting for the staging slot's previous copy (hipEventSynchronize), filling the slot,
    // the hipMemcpyAsync call, hipEventRecord
    double host_ns[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool fail_next = false;            // test hook (cpol_debug_read "fail_next_sweep"): the next launch sequence returns an error
                                       // after its kernels are queued, as a failed copy or capture would
    // sticky domain-error word (device): OR-ed by the kernels of every sweep, cleared only
    // when it has been read AND reported (host-output sweeps, cpol_synchronize, cpol_counters)
    int *d_errword = nullptr;
    int *h_errword = nullptr;          // its page-locked host copy (report_domain_error reads it on the context's own stream: no copy through
                                       // pageable memory, nothing on the null stream)
    std::vector<void *> host_allocs;   // pinned host memory handed out by cpol_host_alloc
    // timing: one event set per sweep since cpol_enable_timing(ctx, 1); elapsed
    // times are collected (averaged) by cpol_counters after the stream drained,
    // so recording does not serialise the timed loop.
    int timing = 0;                    // 0 off, 1 every stage, 2 the PSD stage only
    std::vector<hipEvent_t *> ev_sets;
    size_t ev_used = 0;
    hipEvent_t *ev = nullptr;          // set of the sweep being recorded
    cpol_counters_t counters{};
};

namespace {

// the per-sweep work buffers of cpol_buffers.h, in the order of enum WorkBuf: what run_sequence sizes and fills, the graph key
// mixes, cpol_mem_info counts and cpol_destroy frees
DevBuf cpol_ctx::*const WORK_BUFS[] = {
    &cpol_ctx::b_traj, &cpol_ctx::b_rayc, &cpol_ctx::b_poly, &cpol_ctx::b_timed, &cpol_ctx::b_vals, &cpol_ctx::b_mask, &cpol_ctx::b_elev,
    &cpol_ctx::b_coords, &cpol_ctx::b_wgate, &cpol_ctx::b_qmelt, &cpol_ctx::b_fwmelt,
    &cpol_ctx::b_key, &cpol_ctx::b_pos, &cpol_ctx::b_par, &cpol_ctx::b_count, &cpol_ctx::b_totals, &cpol_ctx::b_blkranked, &cpol_ctx::b_rec,
    &cpol_ctx::b_vmask, &cpol_ctx::b_offset, &cpol_ctx::b_perm, &cpol_ctx::b_res,
    &cpol_ctx::b_vn, &cpol_ctx::b_icefirst, &cpol_ctx::b_proj, &cpol_ctx::b_colin, &cpol_ctx::b_xscr, &cpol_ctx::b_xgeo, &cpol_ctx::b_beam,
    &cpol_ctx::b_bsigma, &cpol_ctx::b_bon,
    &cpol_ctx::b_gscan, &cpol_ctx::b_defer, &cpol_ctx::b_present, &cpol_ctx::b_ticket, &cpol_ctx::b_units, &cpol_ctx::b_szinteg, &cpol_ctx::b_clk};
static_assert(sizeof WORK_BUFS / sizeof WORK_BUFS[0] == WB_N, "cpol_buffers.h: one context member per WorkBuf");

#define HIPCHK(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            char buf_[512];                                                               \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                 \
            ctx->err = buf_;                                                              \
            return CPOL_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)

int ensure(cpol_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap && b.p) return CPOL_OK;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;                      // (the buffer is empty and may be sized again by a later, smaller call)
        (void)hipGetLastError();            // reported through the return code: not left behind as the thread's last error
        ctx->err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
        return CPOL_ERR_NOMEM;
    }
    b.cap = want;
    return CPOL_OK;
}

#define ENSURE(buf, bytes)                                   \
    do {                                                     \
        int rc_ = ensure(ctx, (buf), (size_t)(bytes));       \
        if (rc_ != CPOL_OK) return rc_;                      \
    } while (0)

int upload(cpol_ctx *ctx, DevBuf &b, const void *src, size_t bytes)
{
    ENSURE(b, bytes);
    HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return CPOL_OK;
}

void free_buf(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

int build_itabs(cpol_ctx *ctx);

}  // namespace

namespace {

// Integral tables of every slot whose N(D) has one shape parameter (cpol_device.h: ItabDev).
// Runs after staging, before the first sweep / fork: the PSD kernels integrate one synthetic
// item (N0 = QM = 1) per (LUT slice, lambda panel, Chebyshev node); k_itab_fit turns the 11 node
// values of every (slice, panel, function) into polynomial coefficients.  CPOL_ITAB=0 disables
// (every item is then integrated bin by bin, as in round 1).
int build_itabs(cpol_ctx *ctx)
{
    if (ctx->parent) return CPOL_OK;                      // lanes copy the parent's tables
    if (ctx->itab_serial == ctx->lut_serial) return CPOL_OK;
    const bool enabled = !(getenv("CPOL_ITAB") && atoi(getenv("CPOL_ITAB")) == 0);   // read at every (re)build
    (void)hipGetLastError();            // a stale error of another user of the runtime in this thread is not ours
    ctx->its = ItabSet{};
    ctx->itab_serial = ctx->lut_serial;
    ctx->itab_builds++;
    for (int j = 0; j < CPOL_MAX_HYDRO; ++j) {
        ctx->itab_check[j] = ctx->itab_check_at[j] = ctx->itab_bad[j] = ctx->itab_check_edge[j] = 0.0;
        ctx->itab_ms[j][0] = ctx->itab_ms[j][1] = 0.0;
    }
    if (!enabled) return CPOL_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int n_hyd = ctx->hs.n_hydro;
    constexpr int NC = CPOL_ITAB_NC, NC1 = CPOL_ITAB1_NC;
    // M[pw][q] = sum_n c2m[n][pw] w_n T_n(x_q): node values -> monomial coefficients, for n nodes:
    // out = [M | Tm (nodes -> Chebyshev) | C2M (T_n -> monomials)], each [n][n]
    auto basis_matrices = [](int n, std::vector<double> &out) {
        std::vector<long double> T((size_t)n * n, 0.0L);          // T[k][pw]: monomial coefficients of T_k
        T[0] = 1.0L;
        if (n > 1) T[(size_t)n + 1] = 1.0L;
        for (int k = 2; k < n; ++k)
            for (int pw = 0; pw < n; ++pw)
                T[(size_t)k * n + pw] = (pw > 0 ? 2.0L * T[(size_t)(k - 1) * n + pw - 1] : 0.0L) - T[(size_t)(k - 2) * n + pw];
        const long double pi = 3.141592653589793238462643383279502884L;
        out.assign((size_t)3 * n * n, 0.0);
        for (int pw = 0; pw < n; ++pw)
            for (int q = 0; q < n; ++q) {
                long double acc = 0.0L;
                for (int k = 0; k < n; ++k)
                    acc += T[(size_t)k * n + pw] * (k == 0 ? 1.0L : 2.0L) / n * cosl(pi * k * (q + 0.5L) / n);
                out[(size_t)pw * n + q] = (double)acc;
                out[(size_t)n * n + pw * n + q] = (double)((pw == 0 ? 1.0L : 2.0L) / n * cosl(pi * pw * (q + 0.5L) / n));
                out[(size_t)2 * n * n + pw * n + q] = (double)T[(size_t)pw * n + q];
            }
    };
    {
        std::vector<double> M2, M1;
        basis_matrices(NC, M2);                                    // 2-D blocks (k_itab_fit2: Tm, C2M)
        basis_matrices(NC1, M1);                                   // 1-D blocks (k_itab_fit: M)
        int rc = upload(ctx, ctx->d_itab_M, M2.data(), M2.size() * sizeof(double));
        if (rc != CPOL_OK) return rc;
        rc = upload(ctx, ctx->d_itab_M1, M1.data(), M1.size() * sizeof(double));
        if (rc != CPOL_OK) return rc;
        HIPCHK(hipStreamSynchronize(st));
    }
    const bool melt_enabled = !(getenv("CPOL_ITAB_MELT") && atoi(getenv("CPOL_ITAB_MELT")) == 0);
    // accepted deviation of a block's polynomial from the integrating kernel at the block's check point
    // (CPOL_ITAB_MAX_DEV: test knob -- a tiny value forces the fallback to the integrating kernels)
    const double max_dev = getenv("CPOL_ITAB_MAX_DEV") ? atof(getenv("CPOL_ITAB_MAX_DEV")) : CPOL_ITAB_MAX_DEVIATION;
    const bool dop2 = [&] { for (int j = 0; j < n_hyd; ++j) if (!ctx->hs.h[j].rcsw) return false; return n_hyd > 0; }();
    for (int j = 0; j < n_hyd; ++j) {
        const HydroDev &h = ctx->hs.h[j];
        const cpol_hydro_desc &d = h.d;
        const bool gamma = d.psd_family == CPOL_PSD_GAMMA && h.pre && h.dnu;
        const bool ice = d.psd_family == CPOL_PSD_ICE_FIELD && d.uniform_grid && d.tab_degree == CPOL_ICE_DEGREE;
        const bool melt = d.psd_family == CPOL_PSD_MELTING && melt_enabled;
        if (!gamma && !ice && !melt) continue;
        if (d.table_id) {
            bool hit = false;
            for (auto &e : ctx->itab_cache)
                if (e.id == d.table_id && e.dop2 == (int)dop2) {
                    ctx->its.t[j] = e.t;
                    ctx->itab_check[j] = e.check;
                    ctx->itab_check_edge[j] = e.check_edge;
                    ctx->itab_check_at[j] = e.check_at;
                    e.used = ctx->itab_builds;
                    hit = true;
                    break;
                }
            if (hit) continue;
        }
        // lambda range: 2^-10 .. the lambda at which exp(-lambda D_0^nu) leaves the double range
        // (gamma), resp. the end of the ice normalisation tables
        double d0 = 0.0, lo = -10.0, hi = 15.0;
        if (gamma) {
            HIPCHK(hipMemcpy(&d0, h.dnu, sizeof d0, hipMemcpyDeviceToHost));
            if (!(d0 > 0.0)) continue;
            hi = floor(log2(690.0 / d0) * CPOL_ITAB_PPO) / CPOL_ITAB_PPO;     // whole panels
            if (hi > 16.0) hi = 16.0;
            if (hi <= lo) continue;
        }
        if (melt) {
            // slope of the rain partner, lambda_r = (factor / QM)^(1/(4+mu)): 2^-1 (QM = 0.05 kg m-3) ..
            // 2^8.5 (3e-14: trilinear interpolation towards an empty model cell leaves such values);
            // items beyond are integrated
            lo = -1.0; hi = 8.5;
        }
        const int ppo = melt ? CPOL_ITAB2_PPO : CPOL_ITAB_PPO;
        const int n_pan = (int)floor((hi - lo) * ppo + 0.5);
        const int n_slices = d.n_e * d.n_t;
        const int per_block = melt ? CPOL_ITAB2_NODES : CPOL_ITAB1_NODES;      // the nodes + 1 check point
        const long n_items = (long)n_slices * n_pan * per_block;
        const bool melt_tab = melt && d.tab_degree == CPOL_MELT_DEGREE;
        const int unit_items = ((gamma && d.uniform_grid) || ice || melt_tab) ? 128 : 64;
        const int upers = (n_pan * per_block + unit_items - 1) / unit_items;
        const long n_units = (long)n_slices * upers;
        if (n_items >= (1L << 31)) continue;
        const size_t tab_bytes = (size_t)n_slices * n_pan * (melt ? CPOL_ITAB2_NB : NC1) * CPOL_ITAB_NFP * sizeof(double);
        DevBuf b_par, b_perm, b_units, b_tot, b_res, b_vn, b_det;
        std::vector<unsigned long long> det_bits;
        int rc;
        // destination: the slot's own buffers, or (table_id given) a cache entry of its own
        ItabCacheEntry *ce = nullptr;
        if (d.table_id) {
            if (ctx->itab_cache.size() >= CPOL_ITAB_CACHE) {          // evict the least recently used
                size_t victim = ctx->itab_cache.size();
                for (size_t k = 0; k < ctx->itab_cache.size(); ++k)
                    if (ctx->itab_cache[k].used != ctx->itab_builds &&
                        (victim == ctx->itab_cache.size() || ctx->itab_cache[k].used < ctx->itab_cache[victim].used))
                        victim = k;
                if (victim < ctx->itab_cache.size()) {
                    free_buf(ctx->itab_cache[victim].tab);
                    free_buf(ctx->itab_cache[victim].head);
                    ctx->itab_cache.erase(ctx->itab_cache.begin() + victim);
                }
            }
            if (ctx->itab_cache.size() < CPOL_ITAB_CACHE) {
                ctx->itab_cache.emplace_back();
                ce = &ctx->itab_cache.back();
                ce->id = d.table_id; ce->dop2 = (int)dop2; ce->used = ctx->itab_builds;
            }
        }
        DevBuf &dst_tab = ce ? ce->tab : ctx->d_itab[j];
        DevBuf &dst_head = ce ? ce->head : ctx->d_itab_head[j];
        auto drop_entry = [&] { if (ce) { free_buf(ce->tab); free_buf(ce->head); ctx->itab_cache.pop_back(); ce = nullptr; } };
        if (melt) {
            // centre and 1 / half-width of the wet-fraction bins of the table's second axis; bin 0
            // reaches down to fw = 0 and the last bin up to 1 (lut.py:336-341 clips the index)
            std::vector<double> head(2 * (size_t)d.n_t);
            for (int b = 0; b < d.n_t; ++b) {
                const double blo = b == 0 ? 0.0 : (double)d.t_lo + b * (double)d.t_step;
                const double bhi = b == d.n_t - 1 ? 1.0 : (double)d.t_lo + (b + 1) * (double)d.t_step;
                head[2 * b] = 0.5 * (blo + bhi);
                head[2 * b + 1] = 1.0 / (0.5 * (bhi - blo));
            }
            if ((rc = upload(ctx, dst_head, head.data(), head.size() * sizeof(double)))) { drop_entry(); return rc; }
            HIPCHK(hipStreamSynchronize(st));
        }
        if ((rc = ensure(ctx, b_par, (size_t)CPOL_MAX_PAR * n_items * sizeof(double))) ||
            (rc = ensure(ctx, b_perm, (size_t)n_items * sizeof(int))) ||
            (rc = ensure(ctx, b_units, (size_t)n_units * sizeof(WorkUnit))) ||
            (rc = ensure(ctx, b_tot, 8 * sizeof(long long))) ||
            (rc = ensure(ctx, b_res, (size_t)n_items * CPOL_N_SZ * sizeof(double))) ||
            (rc = ensure(ctx, b_vn, (size_t)n_items * 2 * sizeof(double))) ||
            (rc = ensure(ctx, b_det, (size_t)(2 * n_pan + CPOL_ITAB_NF) * sizeof(unsigned long long))) ||
            (rc = ensure(ctx, dst_tab, tab_bytes))) {
            free_buf(b_par); free_buf(b_perm); free_buf(b_units); free_buf(b_tot); free_buf(b_res); free_buf(b_vn); free_buf(b_det);
            drop_entry();
            return rc;
        }
        HIPCHK(hipMemsetAsync(b_vn.p, 0, (size_t)n_items * 2 * sizeof(double), st));
        ItabBuildArgs ba{};
        ba.par = (double *)b_par.p; ba.perm = (int *)b_perm.p; ba.units = (WorkUnit *)b_units.p;
        ba.totals = (long long *)b_tot.p; ba.n_items = n_items; ba.n_slices = n_slices; ba.n_pan = n_pan;
        ba.key_base = h.key_base; ba.unit_items = unit_items; ba.log2_lo = lo; ba.ppo = ppo;
        ba.two_d = melt ? 1 : 0; ba.n_t = d.n_t; ba.head = (const double *)dst_head.p;
        hipEvent_t evb[4] = {nullptr, nullptr, nullptr, nullptr};
        for (auto &e_ : evb) (void)hipEventCreate(&e_);
        (void)hipEventRecord(evb[0], st);
        hipLaunchKernelGGL(k_itab_nodes, dim3(cdiv(n_items > n_units ? n_items : n_units, 256)), dim3(256), 0, st, ba);
        // the slot's own kernels on the synthetic items (arrays of THIS slot only: the kernels
        // index [n_hydro][...][n] arrays with the slot number, hence the shifted bases)
        PsdArgs pa{};
        pa.units = (const WorkUnit *)b_units.p;
        pa.totals = (const long long *)b_tot.p;
        pa.perm = (const int *)b_perm.p;
        pa.par = (const double *)b_par.p - (long)j * CPOL_MAX_PAR * n_items;
        pa.res = (double *)b_res.p - (long)j * n_items * CPOL_N_SZ;
        pa.vn = (double *)b_vn.p - (long)j * n_items * 2;
        pa.par_w = (double *)b_par.p - (long)j * CPOL_MAX_PAR * n_items;
        pa.n_sbg = n_items;
        pa.clk = nullptr;
        pa.ice_force_sum = 0;
        const dim3 grd((unsigned)(n_units < 4096 ? n_units : 4096)), blk(CPOL_PSD_THREADS);
        if (melt) {
            if (melt_tab) {
                if (dop2) hipLaunchKernelGGL((k_psd_melting_tab<true>), grd, blk, 0, st, ctx->hs, pa);
                else hipLaunchKernelGGL((k_psd_melting_tab<false>), grd, blk, 0, st, ctx->hs, pa);
            } else {
                if (dop2) hipLaunchKernelGGL((k_psd<PSD_MODE_MELTING, true>), grd, blk, 0, st, ctx->hs, pa);
                else hipLaunchKernelGGL((k_psd<PSD_MODE_MELTING, false>), grd, blk, 0, st, ctx->hs, pa);
            }
        } else if (ice) {
            if (dop2) { hipLaunchKernelGGL((k_psd_ice2<true>), grd, blk, 0, st, ctx->hs, pa);
                        hipLaunchKernelGGL((k_psd<PSD_MODE_ICE, true>), grd, blk, 0, st, ctx->hs, pa); }
            else { hipLaunchKernelGGL((k_psd_ice2<false>), grd, blk, 0, st, ctx->hs, pa);
                   hipLaunchKernelGGL((k_psd<PSD_MODE_ICE, false>), grd, blk, 0, st, ctx->hs, pa); }
        } else if (d.uniform_grid) {
            if (dop2) hipLaunchKernelGGL((k_psd_uniform<true>), grd, dim3(CPOL_PSD_THREADS_U), 0, st, ctx->hs, pa);
            else hipLaunchKernelGGL((k_psd_uniform<false>), grd, dim3(CPOL_PSD_THREADS_U), 0, st, ctx->hs, pa);
        } else {
            if (dop2) hipLaunchKernelGGL((k_psd<PSD_MODE_GAMMA_EXP, true>), grd, blk, 0, st, ctx->hs, pa);
            else hipLaunchKernelGGL((k_psd<PSD_MODE_GAMMA_EXP, false>), grd, blk, 0, st, ctx->hs, pa);
        }
        double worst = 0.0;
        unsigned long long worst_bits = 0, edge_bits = 0;
        unsigned int n_bad = 0;
        if (melt) {
            ItabFit2Args fa{};
            fa.res = (const double *)b_res.p; fa.vn = (const double *)b_vn.p;
            fa.M = (const double *)ctx->d_itab_M.p; fa.tab = (double *)dst_tab.p;
            fa.n_blocks = (long)n_slices * n_pan;
            fa.worst = (unsigned long long *)b_tot.p + 3;
            HIPCHK(hipMemsetAsync(fa.worst, 0, sizeof(unsigned long long), st));
            hipLaunchKernelGGL(k_itab_fit2, dim3(cdiv(fa.n_blocks * CPOL_ITAB_NFP, 64)), dim3(64), 0, st, fa);
            (void)hipEventRecord(evb[1], st);
            hipLaunchKernelGGL(k_itab_check2, dim3(cdiv(fa.n_blocks * (CPOL_N_SZ + 2), 256)), dim3(256), 0, st, fa);
            (void)hipEventRecord(evb[2], st);
            HIPCHK(hipMemcpyAsync(&worst_bits, fa.worst, sizeof worst_bits, hipMemcpyDeviceToHost, st));
        } else {
            ItabFitArgs fa{};
            fa.res = (const double *)b_res.p; fa.vn = (const double *)b_vn.p; fa.par = (const double *)b_par.p;
            fa.M = (const double *)ctx->d_itab_M1.p; fa.tab = (double *)dst_tab.p;
            fa.n_items = n_items; fa.n_slices = n_slices; fa.n_pan = n_pan; fa.log2_lo = lo; fa.d0 = gamma ? d0 : 0.0;
            fa.worst = (unsigned long long *)b_tot.p + 3;
            fa.n_bad = (unsigned int *)((unsigned long long *)b_tot.p + 4);
            fa.max_dev = max_dev;
            HIPCHK(hipMemsetAsync(b_det.p, 0, (size_t)(2 * n_pan + CPOL_ITAB_NF) * sizeof(unsigned long long), st));
            fa.by_fn = (unsigned long long *)b_det.p;
            fa.by_pan = fa.by_fn + CPOL_ITAB_NF;            // [n_pan] both check points, then [n_pan] the edge point alone
            det_bits.resize((size_t)2 * n_pan + CPOL_ITAB_NF);
            HIPCHK(hipMemsetAsync(fa.worst, 0, 3 * sizeof(unsigned long long), st));      // worst, n_bad, worst at the edge point
            const dim3 fgrid(cdiv((long)n_slices * n_pan * CPOL_ITAB_NF, 256));
            // (the check is part of the fit kernel: its share of the build = the two check items of every block)
            (void)hipEventRecord(evb[1], st);
            (void)hipEventRecord(evb[2], st);
            hipLaunchKernelGGL(k_itab_fit, fgrid, dim3(256), 0, st, fa);
            HIPCHK(hipMemcpyAsync(&worst_bits, fa.worst, sizeof worst_bits, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(&n_bad, fa.n_bad, sizeof n_bad, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(&edge_bits, fa.worst + 2, sizeof edge_bits, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(det_bits.data(), b_det.p, det_bits.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        }
        (void)hipEventRecord(evb[3], st);
        const hipError_t e = hipStreamSynchronize(st);
        {
            float ms_all = 0.f, ms_chk = 0.f;
            if (e == hipSuccess && hipEventElapsedTime(&ms_all, evb[0], evb[3]) == hipSuccess &&
                hipEventElapsedTime(&ms_chk, evb[1], evb[2]) == hipSuccess) {
                // the check = its kernel + the block's extra item in the integration (1 of per_block)
                ctx->itab_ms[j][0] = ms_all;
                ctx->itab_ms[j][1] = ms_chk + (ms_all - ms_chk) / per_block;
            }
            for (auto &e_ : evb) if (e_) (void)hipEventDestroy(e_);
        }
        free_buf(b_par); free_buf(b_perm); free_buf(b_units); free_buf(b_tot); free_buf(b_res); free_buf(b_vn); free_buf(b_det);
        ctx->itab_detail[j].clear();
        if (!det_bits.empty()) {
            ctx->itab_detail[j] = {lo, (double)ppo, gamma ? d0 : 0.0, (double)n_pan};     // (+ [pan_lo, pan_hi) at the end)
            for (unsigned long long b : det_bits) { double v; memcpy(&v, &b, sizeof v); ctx->itab_detail[j].push_back(v); }
        }
        if (e != hipSuccess || hipGetLastError() != hipSuccess) {
            ctx->err = "build_itabs: a kernel failed";
            drop_entry();
            return CPOL_ERR_HIP;
        }
        {
            const unsigned long long eb = worst_bits & ~0xFFFFFFull;
            memcpy(&worst, &eb, sizeof worst);
            ctx->itab_check_at[j] = (double)(worst_bits & 0xFFFFFFull);      // (block x functions + function) mod 2^24
        }
        ctx->itab_check[j] = worst;
        ctx->itab_bad[j] = (double)n_bad;
        { double ev = 0.0; memcpy(&ev, &edge_bits, sizeof ev); ctx->itab_check_edge[j] = ev; }   // (all panels; the accepted run: below)
        int pan_lo = 0, pan_hi = n_pan;
        // CPOL_ITAB_KEEP_PANELS=<lo>:<hi> (test knob, 1-D tables): only the panels [lo, hi) stay on the table -- the items
        // beyond go to the integrating kernels, as with a table that lost panels to the accuracy gate
        int keep_lo = 0, keep_hi = n_pan;
        if (!melt && getenv("CPOL_ITAB_KEEP_PANELS") && sscanf(getenv("CPOL_ITAB_KEEP_PANELS"), "%d:%d", &keep_lo, &keep_hi) == 2) {
            keep_lo = std::max(0, std::min(keep_lo, n_pan));
            keep_hi = std::max(keep_lo, std::min(keep_hi, n_pan));
        } else { keep_lo = 0; keep_hi = n_pan; }
        if (!melt && !(worst < max_dev)) {
            // 1-D table: keep the longest run of lambda panels whose blocks all pass (in practice everything
            // but the last panel, where exp(-lambda D^nu) of the bins behind the first one goes subnormal);
            // items with lambda outside the run are integrated bin by bin like items outside the table
            const std::vector<double> &dv = ctx->itab_detail[j];
            int best_lo = 0, best_n = 0, run_lo = 0;
            for (int p = 0; p <= n_pan; ++p) {
                const bool ok = p < n_pan && dv[4 + CPOL_ITAB_NF + p] < max_dev;
                if (ok) continue;
                if (p - run_lo > best_n) { best_n = p - run_lo; best_lo = run_lo; }
                run_lo = p + 1;
            }
            if (2 * best_n >= n_pan) {
                pan_lo = best_lo; pan_hi = best_lo + best_n;
                worst = 0.0;
                for (int p = pan_lo; p < pan_hi; ++p) worst = fmax(worst, dv[4 + CPOL_ITAB_NF + p]);
                ctx->itab_check[j] = worst;
            }
        }
        if (!(worst < max_dev)) {
            // the polynomial does not reproduce the integrating kernel between the nodes (melting: wet-
            // fraction bins too wide for the degree, coarse test tables; 1-D: coefficients that cancel):
            // this species stays on the integrating path
            ctx->itab_check[j] = -worst;
            if (ce) drop_entry(); else free_buf(ctx->d_itab[j]);
            continue;
        }
        ItabDev &t = ctx->its.t[j];
        t.tab = (const double *)dst_tab.p;
        t.head = melt ? (const double *)dst_head.p : nullptr;
        t.log2_lo = lo;
        t.d0 = gamma ? d0 : 0.0;
        t.n_pan = n_pan;
        if (!melt) { pan_lo = std::max(pan_lo, keep_lo); pan_hi = std::max(pan_lo, std::min(pan_hi, keep_hi)); }
        t.pan_lo = pan_lo; t.pan_hi = pan_hi;
        if (!ctx->itab_detail[j].empty()) {
            // (the edge point's worst over the accepted run of panels, like `check`)
            const std::vector<double> &dv = ctx->itab_detail[j];
            double we = 0.0;
            for (int p = pan_lo; p < pan_hi; ++p) we = fmax(we, dv[4 + CPOL_ITAB_NF + n_pan + p]);
            ctx->itab_check_edge[j] = we;
            ctx->itab_detail[j].push_back(pan_lo); ctx->itab_detail[j].push_back(pan_hi);
        }
        t.writes_vn = ice || dop2 || d.numeric_intv || melt;
        t.ppo = ppo;
        t.two_d = melt ? 1 : 0;
        t.par_slot = melt ? 2 : 0;
        t.n_t = d.n_t;
        if (ce) { ce->t = t; ce->check = ctx->itab_check[j]; ce->check_at = ctx->itab_check_at[j]; ce->check_edge = ctx->itab_check_edge[j]; }
    }
    return CPOL_OK;
}

}  // namespace

// The range scans keep [3][n_gates] float32 of a ray in dynamic LDS, and a workgroup may ask for 64 KB in all without a kernel
// attribute -- its STATIC part included: k_gate1_ray_scan has 12 bytes of it (s_lookup, s_last, s_done), k_final and k_scan_rays
// none.  CPOL_MAX_GATES (the header) leaves CPOL_SCAN_LDS_STATIC bytes for it, whichever kernel runs the scans; cpol_create
// compares that figure with what the compiler reports for each of them.
#define CPOL_SCAN_LDS_STATIC 16
static_assert((size_t)3 * CPOL_MAX_GATES * sizeof(float) + CPOL_SCAN_LDS_STATIC <= 64 * 1024 &&
              (size_t)3 * (CPOL_MAX_GATES + 1) * sizeof(float) + CPOL_SCAN_LDS_STATIC > 64 * 1024,
              "CPOL_MAX_GATES: the most gates whose three scan rows fit 64 KB of LDS next to the scan kernels' static part");

static bool scan_kernels_fit_lds()
{
    const void *const kernels[4] = {(const void *)k_gate1_ray_scan, (const void *)k_scan_rays, (const void *)k_final<CPOL_FINAL_THREADS>,
                                    (const void *)k_final<2 * CPOL_FINAL_THREADS>};
    for (const void *k : kernels) {
        hipFuncAttributes fa{};
        if (hipFuncGetAttributes(&fa, k) != hipSuccess || fa.sharedSizeBytes > CPOL_SCAN_LDS_STATIC) return false;
    }
    return true;
}

// test hook (cpol_debug_scan): one wavefront per row takes the row through LDS and runs one of the product's two range-scan
// functions on it as they are (cpol_final.inl; both are compiled whatever CPOL_SCAN_FORM says)
template <bool MUL, bool WAVE>
__global__ __launch_bounds__(64) void k_debug_scan(const float *__restrict__ x, float *__restrict__ y, int n)
{
    extern __shared__ float s_dbg_row[];               // [n]
    const int lane = threadIdx.x;
    const long base = (long)blockIdx.x * n;
    for (int g = lane; g < n; g += 64) s_dbg_row[g] = x[base + g];
    __syncthreads();
    if (WAVE) scan_lds_wave_exact<MUL>(s_dbg_row, n, lane);
    else if (lane == 0) scan_lds_sequential<MUL>(s_dbg_row, n);
    __syncthreads();
    for (int g = lane; g < n; g += 64) y[base + g] = s_dbg_row[g];
}

extern "C" {

int cpol_create(int device, cpol_ctx **out)
{
    if (!out) return CPOL_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return CPOL_ERR_HIP;
    cpol_ctx *ctx = new cpol_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return CPOL_ERR_HIP;
    }
    ctx->own_stream = true;
    static const bool scans_fit = scan_kernels_fit_lds();      // (once per process: a build whose scan kernels outgrew CPOL_SCAN_LDS_STATIC)
    if (!scans_fit) {
        (void)hipGetLastError();
        (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return CPOL_ERR_HIP;
    }
    if (getenv("CPOL_ERRWORD") && !strcmp(getenv("CPOL_ERRWORD"), "pageable")) ctx->h_errword = nullptr;      // (measurement knob: round 4's read)
    else if (hipHostMalloc((void **)&ctx->h_errword, 64, hipHostMallocDefault) != hipSuccess) { ctx->h_errword = nullptr; (void)hipGetLastError(); }
    if (hipMalloc((void **)&ctx->d_errword, sizeof(int)) != hipSuccess ||
        hipMemset(ctx->d_errword, 0, sizeof(int)) != hipSuccess) {
        (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return CPOL_ERR_HIP;
    }
    ctx->knobs = knobs_from_env();
    *out = ctx;
    return CPOL_OK;
}

static void stencil_drop_all(cpol_ctx *root);

void cpol_destroy(cpol_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->parent) {
        // staged buffers belong to the parent
        ctx->d_H = DevBuf(); ctx->d_V = DevBuf();
        for (int j = 0; j < CPOL_MAX_HYDRO; ++j) {
            ctx->d_table[j] = DevBuf(); ctx->d_pre[j] = DevBuf(); ctx->d_dnu[j] = DevBuf();
            ctx->d_aux[j] = DevBuf(); ctx->d_rcsw[j] = DevBuf();
            ctx->d_rcs32[j] = DevBuf(); ctx->d_dgrid[j] = DevBuf();
        }
        for (auto &b : ctx->d_tfun) b = DevBuf();
        for (auto &b : ctx->d_itab) b = DevBuf();
        for (auto &b : ctx->d_itab_head) b = DevBuf();
        ctx->d_itab_M = DevBuf(); ctx->d_itab_M1 = DevBuf();
        ctx->parent->n_children -= 1;
    }
    for (auto &b : ctx->d_tfun) free_buf(b);
    for (auto &b : ctx->d_itab) free_buf(b);
    for (auto &b : ctx->d_itab_head) free_buf(b);
    for (auto &e : ctx->itab_cache) { free_buf(e.tab); free_buf(e.head); }
    ctx->itab_cache.clear();
    for (auto &e : ctx->table_cache) free_buf(e.buf);
    ctx->table_cache.clear();
    free_buf(ctx->d_itab_M);
    free_buf(ctx->d_itab_M1);
    for (int i = 0; i < 3; ++i) {
        if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
        if (ctx->aux[i]) { (void)hipStreamSynchronize(ctx->aux[i]); (void)hipStreamDestroy(ctx->aux[i]); }
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    for (auto &sg : ctx->stg) {
        if (sg.ev) (void)hipEventDestroy(sg.ev);
        if (sg.p) (void)hipHostFree(sg.p);
    }
    for (auto &ts : ctx->tsets) { free_buf(ts.buf); free_buf(ts.poly); }
    if (!ctx->parent) stencil_drop_all(ctx);                         // (the gate stencils)
    free_buf(ctx->d_hdiff);
    if (!ctx->parent) for (auto &b : ctx->members) free_buf(b);      // (the cubes of the ensemble members)
    ctx->members.clear();
    for (DevBuf cpol_ctx::*m : WORK_BUFS) free_buf(ctx->*m);       // the per-sweep work buffers (cpol_buffers.h)
    DevBuf *rest[] = {&ctx->d_H, &ctx->d_V, &ctx->d_geoM, &ctx->b_spectrum, &ctx->b_outwin, &ctx->b_superob, &ctx->b_smom, &ctx->b_smcount,
                      &ctx->b_smvar, &ctx->b_hstate, &ctx->b_hedges, &ctx->b_cstate, &ctx->b_cedges, &ctx->b_crays, &ctx->b_cplane,
                      &ctx->b_fsat, &ctx->b_fobs, &ctx->b_oscr, &ctx->b_fmaps, &ctx->b_mstate, &ctx->b_msout, &ctx->b_mstash, &ctx->b_mvobs,
                      &ctx->b_rvel, &ctx->b_sztotal, &ctx->b_model, &ctx->b_mask8, &ctx->b_vis};
    for (DevBuf *b : rest) free_buf(*b);
    for (auto &b : ctx->b_hcounts) free_buf(b);
    for (auto &b : ctx->b_spout) free_buf(b);
    for (auto &b : ctx->b_cout) free_buf(b);
    for (auto &b : ctx->b_fout) free_buf(b);
    free_buf(ctx->b_ctab);
    free_buf(ctx->b_cwtab);
    for (auto &cp : ctx->cplanes) free_buf(cp.buf);
    for (auto &b : ctx->b_out) free_buf(b);
    for (int j = 0; j < CPOL_MAX_HYDRO; ++j) {
        free_buf(ctx->d_table[j]);
        free_buf(ctx->d_pre[j]);
        free_buf(ctx->d_dnu[j]);
        free_buf(ctx->d_aux[j]);
        free_buf(ctx->d_rcsw[j]);
        free_buf(ctx->d_rcs32[j]);
        free_buf(ctx->d_dgrid[j]);
    }
    for (hipEvent_t *set : ctx->ev_sets) {
        for (int k = 0; k < EV_N; ++k) (void)hipEventDestroy(set[k]);
        delete[] set;
    }
    for (hipGraphExec_t g : ctx->graph_exec) if (g) (void)hipGraphExecDestroy(g);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->d_errword) (void)hipFree(ctx->d_errword);
    if (ctx->h_errword) (void)hipHostFree(ctx->h_errword);
    for (void *h : ctx->host_allocs) (void)hipHostFree(h);
    delete ctx;
}

int cpol_fork(cpol_ctx *parent, cpol_ctx **out)
{
    if (!out) return CPOL_ERR_ARG;
    *out = nullptr;
    if (!parent || parent->parent) {
        if (parent) parent->err = "cpol_fork: fork the root context, not a lane";
        return CPOL_ERR_ARG;
    }
    cpol_ctx *ctx = parent;            // for HIPCHK
    HIPCHK(hipSetDevice(parent->device));
    HIPCHK(hipStreamSynchronize(parent->stream));      // staging has landed
    cpol_ctx *c = new cpol_ctx();
    c->device = parent->device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        parent->err = "cpol_fork: hipStreamCreate failed";
        return CPOL_ERR_HIP;
    }
    c->own_stream = true;
    c->h_errword = nullptr;
    if (parent->h_errword && hipHostMalloc((void **)&c->h_errword, 64, hipHostMallocDefault) != hipSuccess) { c->h_errword = nullptr; (void)hipGetLastError(); }
    if (hipMalloc((void **)&c->d_errword, sizeof(int)) != hipSuccess ||
        hipMemset(c->d_errword, 0, sizeof(int)) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        parent->err = "cpol_fork: hipMalloc failed";
        return CPOL_ERR_NOMEM;
    }
    c->knobs = parent->knobs;
    c->parent = parent;
    c->model_staged = parent->model_staged;
    c->model = parent->model;
    c->member_sel = parent->member_sel;
    c->hs = parent->hs;
    c->ss = parent->ss;
    for (int j = 0; j < CPOL_MAX_HYDRO; ++j) c->hydro_staged[j] = parent->hydro_staged[j];
    for (int k = 0; k < CPOL_N_TFUN; ++k) c->tfun[k] = parent->tfun[k];
    {   // the parent's integral tables are complete before any lane exists
        const int rc_it = build_itabs(parent);
        if (rc_it != CPOL_OK) { (void)hipStreamDestroy(c->stream); (void)hipFree(c->d_errword); delete c; return rc_it; }
    }
    c->its = parent->its;
    c->itab_serial = parent->lut_serial;
    parent->n_children += 1;
    *out = c;
    return CPOL_OK;
}

const char *cpol_last_error(cpol_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int cpol_set_stream(cpol_ctx *ctx, void *hip_stream)
{
    if (!ctx) return CPOL_ERR_ARG;
    ctx->st_seen.clear();               // (gate stencils: another stream has waited for no recording launch yet)
    if (ctx->own_stream) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamDestroy(ctx->stream);
        ctx->own_stream = false;
    }
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    return CPOL_OK;
}

int cpol_get_stream(cpol_ctx *ctx, void **hip_stream)
{
    if (!ctx || !hip_stream) return CPOL_ERR_ARG;
    *hip_stream = (void *)ctx->stream;
    return CPOL_OK;
}

// reads the sticky domain-error word (the stream has drained); a set word is cleared and
// reported ONCE as CPOL_ERR_DOMAIN -- so a sweep that left the model domain is never lost
// behind later sweeps of the same context (the reference raises IndexError at that radial)
static int report_domain_error(cpol_ctx *ctx)
{
    // (called behind a hipStreamSynchronize of ctx->stream.  The word travels into page-locked memory on that stream: a
    // blocking hipMemcpy into a stack variable goes through the null stream and the runtime's staging of pageable
    // memory -- after the first of those, the first asynchronous copy of every following sweep took ~340 us with ~200
    // page faults for the next two synchronisation periods: round 4's "slow mode", profiles/r5_host_mode_probe.txt)
    int flag = 0;
    if (ctx->h_errword) {
        HIPCHK(hipMemcpyAsync(ctx->h_errword, ctx->d_errword, sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        flag = *(volatile int *)ctx->h_errword;
    } else {
        HIPCHK(hipMemcpy(&flag, ctx->d_errword, sizeof flag, hipMemcpyDeviceToHost));
    }
    if (!flag) return CPOL_OK;
    HIPCHK(hipMemsetAsync(ctx->d_errword, 0, sizeof(int), ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->err = "RADAR DOMAIN IS NOT ENTIRELY CONTAINED IN COSMO SIMULATION DOMAIN";
    return CPOL_ERR_DOMAIN;
}

int cpol_synchronize(cpol_ctx *ctx)
{
    if (!ctx) return CPOL_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return report_domain_error(ctx);
}

int cpol_host_alloc(cpol_ctx *ctx, size_t bytes, void **out)
{
    if (!out || bytes == 0) return CPOL_ERR_ARG;
    *out = nullptr;
    if (!ctx) {
        // context-free block: owned by the caller until cpol_host_free(NULL, p) (a host-side pool whose
        // blocks outlive the contexts that copy into them)
        void *h = nullptr;
        if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess || !h) return CPOL_ERR_NOMEM;
        *out = h;
        return CPOL_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    void *h = nullptr;
    if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess || !h) {
        ctx->err = "cpol_host_alloc: hipHostMalloc failed";
        return CPOL_ERR_NOMEM;
    }
    ctx->host_allocs.push_back(h);
    *out = h;
    return CPOL_OK;
}

int cpol_host_alloc_near(int device, size_t bytes, void **out)
{
    // a context-free block like cpol_host_alloc(NULL, ...), but placed for `device`: the runtime takes
    // page-locked memory from the NUMA node next to the CURRENT device of the calling thread, which a
    // helper thread of a rank on GPU 5 has never set
    if (!out || bytes == 0 || device < 0) return CPOL_ERR_ARG;
    *out = nullptr;
    int prev = -1, n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); return CPOL_ERR_HIP; }
    if (device >= n_dev) return CPOL_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CPOL_ERR_ARG; }
    void *h = nullptr;
    hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocDefault);
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    if (e != hipSuccess || !h) { (void)hipGetLastError(); return CPOL_ERR_NOMEM; }
    *out = h;
    return CPOL_OK;
}

int cpol_device_pci_bus_id(int device, char *buf, int len)
{
    if (!buf || len < 16 || device < 0) return CPOL_ERR_ARG;
    buf[0] = 0;
    if (hipDeviceGetPCIBusId(buf, len, device) == hipSuccess) return CPOL_OK;
    (void)hipGetLastError();            // (reported through the return code: not left behind as the thread's last error)
    return CPOL_ERR_HIP;
}

int cpol_mem_info(cpol_ctx *ctx, size_t *free_bytes, size_t *total_bytes, size_t *per_gate)
{
    if (!ctx) return CPOL_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    // "free" for a launch sequence of THIS context = what the device has free + what the context's grow-only work
    // buffers hold already (a scan that fitted as one sequence the first time fits again: a caller that sizes its
    // batches by this figure groups the same scan the same way on every call)
    {
        for (int w = 0; w < WB_N; ++w) {
            const DevBuf &b = ctx->*WORK_BUFS[w];
            if (BUF_ROWS[w].held && b.p) f += b.cap;
        }
        if (f > t) f = t;
    }
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    if (per_gate) {
        // the arenas cpol_run_sweep sizes by n_sbg (vals, masks, elevation, melting scratch, per-item key / pos /
        // par / rec / perm / res / vn, velocity terms, per-gate weights)
        const size_t n_hyd = (size_t)(ctx->hs.n_hydro > 0 ? ctx->hs.n_hydro : 1), n_vars = (size_t)(ctx->model.n_vars > 0 ? ctx->model.n_vars : 9);
        *per_gate = buf_per_gate(n_vars, n_hyd);
    }
    return CPOL_OK;
}

int cpol_host_free(cpol_ctx *ctx, void *p)
{
    if (!p) return CPOL_ERR_ARG;
    if (!ctx) return hipHostFree(p) == hipSuccess ? CPOL_OK : CPOL_ERR_HIP;   // a context-free block (see above)
    for (size_t i = 0; i < ctx->host_allocs.size(); ++i)
        if (ctx->host_allocs[i] == p) {
            HIPCHK(hipStreamSynchronize(ctx->stream));      // no copy into it may be in flight
            (void)hipHostFree(p);
            ctx->host_allocs.erase(ctx->host_allocs.begin() + (long)i);
            return CPOL_OK;
        }
    ctx->err = "cpol_host_free: not a cpol_host_alloc pointer of this context";
    return CPOL_ERR_ARG;
}

int cpol_enable_timing(cpol_ctx *ctx, int on)
{
    if (!ctx) return CPOL_ERR_ARG;
    ctx->timing = (on == 2) ? 2 : (on != 0);
    ctx->ev_used = 0;                  // restart the averaging window
    return CPOL_OK;
}

// a model is staged on the context itself, never on a lane, and not while lanes of it exist
static bool model_on_lane(cpol_ctx *ctx, const char *who)
{
    if (!ctx->parent && !ctx->n_children) return false;
    ctx->err = std::string(who) + ": not on a lane, and not while lanes of this context exist (cpol_fork)";
    return true;
}

// ---- gate stencils: the store of the root context ----
// every entry dies (the caller holds no lanes and has drained -- or drains here -- the root's stream)
static void stencil_drop_all(cpol_ctx *root)
{
    (void)hipStreamSynchronize(root->stream);
    std::lock_guard<std::mutex> lk(root->st_mu);
    for (StencilEntry *e : root->st_entries) {
        if (e->buf) (void)hipFree(e->buf);
        if (e->ev) (void)hipEventDestroy(e->ev);
        delete e;
    }
    root->st_drops += root->st_entries.size();
    root->st_entries.clear();
    root->st_bytes = 0;
    root->st_seen.clear();
}

// the level heights, the grid or the rotation are about to change: a new identity, no entry survives
static void stencil_new_heights(cpol_ctx *root)
{
    stencil_drop_all(root);
    root->st_heights++;
}

static void stencil_views(const StencilEntry *e, StencilDev *sd)
{
    char *b = (char *)e->buf;
    const size_t n = (size_t)e->n_pad;
    sd->z1 = (StencilZ *)b;                  b += 16 * n;
    sd->z2 = (StencilZ *)b;                  b += 16 * n;
    sd->cell = (int2 *)b;                    b += 8 * n;
    sd->c1 = (StencilC1 *)b;                 b += 8 * n;
    sd->s = (float *)b;                      b += 4 * n;
    sd->h = (float *)b;                      b += 4 * n;
    sd->e = (float *)b;                      b += 4 * n;
    sd->x = (float *)b;                      b += 4 * n;
    sd->y = (float *)b;                      b += 4 * n;
    sd->status = (signed char *)b;
}

// The form of this sweep's gate kernel: 0 full (first sight of the key: noted; or no room), 1 recording (second sight; *made is the
// entry, published by stencil_recorded once the launch and its event are queued), 2 replay (the stream waits for the recording
// launch's event the first time this context meets the entry).
static int stencil_pick(cpol_ctx *ctx, const StencilKey &key, long n_rg, StencilDev *sd, StencilEntry **made)
{
    cpol_ctx *r = ctx->parent ? ctx->parent : ctx;
    std::lock_guard<std::mutex> lk(r->st_mu);
    if (!r->st_budget) return 0;
    StencilEntry *e = nullptr;
    for (StencilEntry *x : r->st_entries)
        if (memcmp(&x->key, &key, sizeof key) == 0) { e = x; break; }
    if (!e) {
        // first sight: a note (no device memory).  The notes of geometries that never came again do not pile up without bound
        if (r->st_entries.size() >= 4096) {
            for (size_t i = 0; i < r->st_entries.size(); ++i)
                if (r->st_entries[i]->state == 0) { delete r->st_entries[i]; r->st_entries.erase(r->st_entries.begin() + (long)i); break; }
            if (r->st_entries.size() >= 4096) return 0;
        }
        try {
            e = new StencilEntry();
            e->key = key;
            e->id = r->st_next_id++;
            r->st_entries.push_back(e);
        } catch (...) { delete e; }
        return 0;
    }
    if (e->refused || e->state == 1) return 0;
    if (e->state == 0) {
        const long n_pad = (n_rg + 63) & ~63L;
        const size_t bytes = (size_t)n_pad * CPOL_STENCIL_BYTES_PER_GATE;
        if (bytes > r->st_budget || r->st_bytes > r->st_budget - bytes) { e->refused = true; return 0; }
        if (hipMalloc(&e->buf, bytes) != hipSuccess) { (void)hipGetLastError(); e->buf = nullptr; e->refused = true; return 0; }
        if (hipEventCreateWithFlags(&e->ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(e->buf);
            e->buf = nullptr; e->ev = nullptr; e->refused = true;
            return 0;
        }
        e->bytes = bytes; e->n_pad = n_pad; e->state = 1;
        r->st_bytes += bytes;
        stencil_views(e, sd);
        *made = e;
        return 1;
    }
    stencil_views(e, sd);
    bool seen = false;
    for (uint64_t id : ctx->st_seen) seen = seen || id == e->id;
    if (!seen) {
        if (hipStreamWaitEvent(ctx->stream, e->ev, 0) != hipSuccess) { (void)hipGetLastError(); return 0; }
        try { ctx->st_seen.push_back(e->id); } catch (...) { }      // (not remembered: it waits again, harmlessly)
    }
    r->st_replays++;
    return 2;
}

// behind the recording launch: its event, then the entry is there for every lane
static int stencil_recorded(cpol_ctx *ctx, StencilEntry *e)
{
    cpol_ctx *r = ctx->parent ? ctx->parent : ctx;
    const hipError_t rc = hipEventRecord(e->ev, ctx->stream);
    std::lock_guard<std::mutex> lk(r->st_mu);
    if (rc != hipSuccess) { (void)hipGetLastError(); e->refused = true; return 0; }      // (it keeps its memory until the store is dropped)
    e->state = 2;
    r->st_records++;
    try { ctx->st_seen.push_back(e->id); } catch (...) { }
    return 1;
}

// the context bookkeeping behind a freshly written d_H / d_V (cpol_stage_model, cpol_stage_model_packed)
// the cubes of members >= 1 go with the cube they were staged beside (cpol_stage_model, cpol_stage_model_packed, cpol_destroy)
static void drop_members(cpol_ctx *ctx)
{
    for (auto &b : ctx->members) free_buf(b);
    ctx->members.clear();
    ctx->member_sel = 0;
}

static void model_staged_tail(cpol_ctx *ctx, int n_vars, int nz, int ny, int nx, size_t h_bytes, const float llc[2],
                              const float urc[2], const float res[2], const double south_pole[2])
{
    ModelDev &m = ctx->model;
    m.H = (const float *)ctx->d_H.p;
    m.HT = (const float2 *)((const char *)ctx->d_H.p + h_bytes);
    m.V = (const float *)ctx->d_V.p;
    m.n_vars = n_vars; m.nz = nz; m.ny = ny; m.nx = nx;
    m.llc0 = llc[0]; m.llc1 = llc[1];
    m.urc0 = urc[0]; m.urc1 = urc[1];
    m.res0 = res[0]; m.res1 = res[1];
    m.rres0 = 1.0 / (double)m.res0; m.rres1 = 1.0 / (double)m.res1;      // (IEEE division on the host: correctly rounded)
    // rotation constants (oracle/cosmo_pol_oracle/geodesy.py: rotation_constants)
    const double theta = (90.0 + south_pole[0]) * CPOL_DEG, phi = south_pole[1] * CPOL_DEG;
    const double ct = cos(theta), st = sin(theta), cp = cos(phi), sp = sin(phi);
    m.ctcp = ct * cp; m.ctsp = ct * sp; m.st = st; m.nsp = -sp; m.cp = cp;
    m.nstcp = -st * cp; m.stsp = st * sp; m.ct = ct;
    ctx->model_pole[0] = south_pole[0]; ctx->model_pole[1] = south_pole[1];
    ctx->model_staged = true;
    ctx->stage_serial++;
    drop_members(ctx);                  // (a new member 0: the others belonged to the previous one)
    // the coordinate polynomials of the resident table sets hold the PREVIOUS model's rotated-pole matrix (round-5 advisor
    // finding: a second cube with another south pole, the same rays again -> wrong grid cells without an error)
    for (auto &ts : ctx->tsets) ts.poly_version = 0;
}

int cpol_stage_model(cpol_ctx *ctx, int n_vars, const float *const *data, const float *zlevels,
                     int nz, int ny, int nx, const float llc[2], const float urc[2],
                     const float res[2], const double south_pole[2])
{
    if (!ctx || !data || !zlevels || n_vars < 1 || n_vars > CPOL_MAX_VARS || nz < 3 || ny < 2 ||
        nx < 2) {
        if (ctx) ctx->err = "cpol_stage_model: bad arguments (need nz >= 3, ny, nx >= 2)";
        return CPOL_ERR_ARG;
    }
    (void)hipGetLastError();            // a stale error of another user of the runtime in this thread is not ours
    if (model_on_lane(ctx, "cpol_stage_model")) return CPOL_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const long ncell = (long)ny * nx;
    const size_t plane_bytes = (size_t)nz * ncell * sizeof(float);
    const size_t h_bytes = (plane_bytes + 7) & ~(size_t)7;        // + (top, lowest level) per column behind the levels
    // Gate stencils outlive a model load whose heights identity is the resident one: the same grid and pole, bytewise, and level
    // heights that are bit for bit what d_H holds -- compared exactly, by the staging kernel itself as it overwrites them.
    void *const h_was = ctx->d_H.p;
    bool keep_stencils;
    {
        const ModelDev &m0 = ctx->model;
        const float grid_new[6] = {llc[0], llc[1], urc[0], urc[1], res[0], res[1]};
        const float grid_old[6] = {m0.llc0, m0.llc1, m0.urc0, m0.urc1, m0.res0, m0.res1};
        std::lock_guard<std::mutex> lk(ctx->st_mu);
        keep_stencils = ctx->model_staged && !ctx->st_entries.empty() && m0.nz == nz && m0.ny == ny && m0.nx == nx &&
                        memcmp(grid_new, grid_old, sizeof grid_new) == 0 && memcmp(south_pole, ctx->model_pole, 2 * sizeof(double)) == 0;
    }
    if (keep_stencils && ensure(ctx, ctx->d_hdiff, sizeof(int)) != CPOL_OK) keep_stencils = false;
    if (!keep_stencils) stencil_new_heights(ctx);
    // (from here on an early return leaves heights that may be half written: the store goes with them unless the end is reached)
    struct DropUnlessKept {
        cpol_ctx *c; bool armed;
        ~DropUnlessKept() { if (armed) stencil_new_heights(c); }
    } guard{ctx, keep_stencils};
    ENSURE(ctx->d_H, h_bytes + (size_t)ncell * sizeof(float2));
    ENSURE(ctx->d_V, plane_bytes * n_vars);
    if (keep_stencils && ctx->d_H.p != h_was) { stencil_new_heights(ctx); guard.armed = keep_stencils = false; }
    DevBuf tmp;
    int rc = ensure(ctx, tmp, plane_bytes);
    if (rc != CPOL_OK) return rc;
    const int blk = 256, grd = cdiv(ncell, blk);
    int h_differs = 0;
    HIPCHK(hipMemcpyAsync(tmp.p, zlevels, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (keep_stencils) {
        HIPCHK(hipMemsetAsync(ctx->d_hdiff.p, 0, sizeof(int), ctx->stream));
        hipLaunchKernelGGL(k_stage_heights_cmp, dim3(grd), dim3(blk), 0, ctx->stream, (const float *)tmp.p,
                           (float *)ctx->d_H.p, (float2 *)((char *)ctx->d_H.p + h_bytes), nz, ncell, (int *)ctx->d_hdiff.p);
        HIPCHK(hipMemcpyAsync(&h_differs, ctx->d_hdiff.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));   // (read behind the loop's synchronisation)
    } else
    hipLaunchKernelGGL(k_stage_heights, dim3(grd), dim3(blk), 0, ctx->stream, (const float *)tmp.p,
                       (float *)ctx->d_H.p, (float2 *)((char *)ctx->d_H.p + h_bytes), nz, ncell);
    for (int v = 0; v < n_vars; ++v) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpyAsync(tmp.p, data[v], plane_bytes, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_stage_variable, dim3(grd), dim3(blk), 0, ctx->stream,
                           (const float *)tmp.p, (float *)ctx->d_V.p, nz, ncell, n_vars, v);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    free_buf(tmp);
    if (keep_stencils && h_differs == 0) guard.armed = false;      // (otherwise the guard drops the store: another identity)
    model_staged_tail(ctx, n_vars, nz, ny, nx, h_bytes, llc, urc, res, south_pole);
    return CPOL_OK;
}

// ---------------------------------------------------------------- ensemble members
static cpol_ctx *root_of(cpol_ctx *ctx) { return ctx->parent ? ctx->parent : ctx; }

// the cube of member k as the kernels read it, or NULL
static const float *member_cube(cpol_ctx *ctx, int k)
{
    cpol_ctx *r = root_of(ctx);
    if (!r->model_staged || k < 0 || k > (int)r->members.size()) return nullptr;
    return (const float *)(k == 0 ? r->d_V.p : r->members[(size_t)k - 1].p);
}

int cpol_num_members(cpol_ctx *ctx)
{
    if (!ctx) return CPOL_ERR_ARG;
    cpol_ctx *r = root_of(ctx);
    return r->model_staged ? 1 + (int)r->members.size() : 0;
}

int cpol_stage_member(cpol_ctx *ctx, int member, int n_vars, const float *const *data)
{
    if (!ctx) return CPOL_ERR_ARG;
    if (!data || member < 0) { ctx->err = "cpol_stage_member: bad arguments"; return CPOL_ERR_ARG; }
    (void)hipGetLastError();
    if (model_on_lane(ctx, "cpol_stage_member")) return CPOL_ERR_ARG;
    if (!ctx->model_staged) { ctx->err = "cpol_stage_member: stage member 0 first (cpol_stage_model)"; return CPOL_ERR_ARG; }
    const ModelDev &m = ctx->model;
    if (n_vars != m.n_vars) { ctx->err = "cpol_stage_member: n_vars differs from the staged cube's"; return CPOL_ERR_ARG; }
    if (member > (int)ctx->members.size() + 1) {
        ctx->err = "cpol_stage_member: members are staged in order (member <= cpol_num_members)";
        return CPOL_ERR_ARG;
    }
    for (int v = 0; v < n_vars; ++v)
        if (!data[v]) { ctx->err = "cpol_stage_member: a variable pointer is NULL"; return CPOL_ERR_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const long ncell = (long)m.ny * m.nx;
    const size_t plane_bytes = (size_t)m.nz * ncell * sizeof(float);
    const bool fresh = member == (int)ctx->members.size() + 1;
    // (every allocation before the first write: out of memory leaves what was staged before as it was)
    DevBuf tmp;
    int rc = ensure(ctx, tmp, plane_bytes);
    if (rc != CPOL_OK) return rc;
    if (fresh) {
        try { ctx->members.emplace_back(); } catch (...) { free_buf(tmp); ctx->err = "cpol_stage_member: out of host memory"; return CPOL_ERR_NOMEM; }
        // (exactly the cube: the head room `ensure` gives a grow-only work buffer would be 12 % of every member)
        DevBuf &mb = ctx->members.back();
        const hipError_t e = hipMalloc(&mb.p, plane_bytes * n_vars);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ctx->members.pop_back();
            free_buf(tmp);
            ctx->err = std::string("cpol_stage_member: hipMalloc failed: ") + hipGetErrorString(e);
            return CPOL_ERR_NOMEM;
        }
        mb.cap = plane_bytes * n_vars;
    }
    float *const dst = (float *)(member == 0 ? ctx->d_V.p : ctx->members[(size_t)member - 1].p);
    const int blk = 256, grd = cdiv(ncell, blk);
    for (int v = 0; v < n_vars; ++v) {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tmp.p, data[v], plane_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            if (fresh) { free_buf(ctx->members.back()); ctx->members.pop_back(); }
            free_buf(tmp);
            ctx->err = std::string("cpol_stage_member: copy failed: ") + hipGetErrorString(e);
            return CPOL_ERR_HIP;
        }
        hipLaunchKernelGGL(k_stage_variable, dim3(grd), dim3(blk), 0, ctx->stream, (const float *)tmp.p, dst, m.nz, ncell, n_vars, v);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    free_buf(tmp);
    // (kernel arguments of a captured graph may hold this cube: the key changes.  The scattering and integral tables do not
    // depend on the model: lut_serial stays)
    ctx->stage_serial++;
    return CPOL_OK;
}

int cpol_select_member(cpol_ctx *ctx, int member)
{
    if (!ctx) return CPOL_ERR_ARG;
    const float *V = member_cube(ctx, member);
    if (!V) { ctx->err = "cpol_select_member: no such member staged"; return CPOL_ERR_ARG; }
    // ModelDev travels to the kernels by value: the next launch reads the other cube.  What is keyed by the cube -- the
    // captured HIP graph -- is keyed by stage_serial; the coordinate polynomials and per-ray tables depend on the grid alone
    if (ctx->model.V != V) ctx->stage_serial++;
    ctx->model.V = V;
    ctx->member_sel = member;
    return CPOL_OK;
}

// ---------------------------------------------------------------- packed (GRIB-1) model input
namespace {

size_t packed_slot(const cpol_packed_plane &p) { return p.n_bits ? (((size_t)p.n_octets + 8 + 15) & ~(size_t)15) : 0; }

const char *packed_plane_fault(const cpol_packed_plane &p, long ncell)
{
    if (p.n_bits < 0 || p.n_bits > 32) return "n_bits outside 0 ... 32";
    if (p.n_bits && (!p.octets || p.n_octets < 0 || (unsigned long long)p.n_octets * 8ull < (unsigned long long)ncell * (unsigned)p.n_bits))
        return "fewer octets than ny * nx * n_bits bits";
    if (p.dec_scale < -300 || p.dec_scale > 300 || p.bin_scale < -32767 || p.bin_scale > 32767) return "scale factor out of range";
    return nullptr;
}

// The octets of every plane into one device arena, each bit string at a 16-byte-aligned start with >= 8 octets of slack
// behind it (k_grib_unpack reads whole words), and the descriptor table in one upload.  The caller's (pageable, usually
// file-mapped) memory goes to the runtime's own staging, one copy per plane: page-locked bounce buffers filled by memcpy
// were 5 % slower.
int upload_packed(cpol_ctx *ctx, const cpol_packed_plane *planes, int n, const std::vector<long> &out_plane,
                  DevBuf &arena, DevBuf &desc)
{
    std::vector<PackedPlaneDev> pd((size_t)n);
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        const cpol_packed_plane &p = planes[i];
        PackedPlaneDev &d = pd[(size_t)i];
        d.off = total;
        d.ref = p.ref_value;
        d.dec = 1.0;
        for (int j = 0; j < (p.dec_scale < 0 ? -p.dec_scale : p.dec_scale); ++j) d.dec *= 10.0;
        d.bin_scale = p.bin_scale;
        d.dec_sign = (p.dec_scale > 0) - (p.dec_scale < 0);
        d.n_bits = p.n_bits;
        d.flip = p.flip_rows != 0;
        d.out_plane = out_plane[(size_t)i];
        total += packed_slot(p);
    }
    ENSURE(arena, total + 16);
    int rc = upload(ctx, desc, pd.data(), pd.size() * sizeof(PackedPlaneDev));
    if (rc != CPOL_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (planes[i].n_bits)
            HIPCHK(hipMemcpyAsync((char *)arena.p + pd[(size_t)i].off, planes[i].octets, (size_t)planes[i].n_octets,
                                  hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));      // (pd is this function's: nothing may read it afterwards)
    return CPOL_OK;
}

void launch_unpack(cpol_ctx *ctx, const DevBuf &arena, const DevBuf &desc, float *out, int n, int ny, int nx)
{
    const long ncell = (long)ny * nx;
    for (int first = 0; first < n; first += 32768) {           // (grid.y <= 65535)
        const int m = n - first < 32768 ? n - first : 32768;
        hipLaunchKernelGGL(k_grib_unpack, dim3((unsigned)cdiv(ncell, 256), (unsigned)m), dim3(256), 0, ctx->stream,
                           (const unsigned *)arena.p, (const PackedPlaneDev *)desc.p + first, out, ny, nx);
    }
}

double wall_ms()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return 1e3 * (double)ts.tv_sec + 1e-6 * (double)ts.tv_nsec;
}

}  // namespace

int cpol_unpack_planes(cpol_ctx *ctx, const cpol_packed_plane *planes, int n_planes, int ny, int nx, float *out)
{
    if (!ctx || !planes || !out || n_planes < 1 || ny < 1 || nx < 1 || (long)ny * nx >= (1L << 31)) {
        if (ctx) ctx->err = "cpol_unpack_planes: bad arguments";
        return CPOL_ERR_ARG;
    }
    const long ncell = (long)ny * nx;
    std::vector<long> out_plane((size_t)n_planes);
    for (int i = 0; i < n_planes; ++i) {
        const char *why = packed_plane_fault(planes[i], ncell);
        if (why) { ctx->err = std::string("cpol_unpack_planes: plane ") + std::to_string(i) + ": " + why; return CPOL_ERR_ARG; }
        out_plane[(size_t)i] = i;
    }
    (void)hipGetLastError();            // a stale error of another user of the runtime in this thread is not ours
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf arena, desc, cube;
    const size_t cube_bytes = (size_t)n_planes * ncell * sizeof(float);
    int rc = ensure(ctx, cube, cube_bytes);
    if (rc == CPOL_OK) rc = upload_packed(ctx, planes, n_planes, out_plane, arena, desc);
    if (rc == CPOL_OK) {
        launch_unpack(ctx, arena, desc, (float *)cube.p, n_planes, ny, nx);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out, cube.p, cube_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { ctx->err = std::string("cpol_unpack_planes: ") + hipGetErrorString(e); rc = CPOL_ERR_HIP; }
    }
    free_buf(arena); free_buf(desc); free_buf(cube);
    return rc;
}

int cpol_stage_model_packed(cpol_ctx *ctx, const cpol_packed_model *m, const cpol_packed_plane *planes, int n_planes)
{
    if (!ctx || !m || !planes) {
        if (ctx) ctx->err = "cpol_stage_model_packed: bad arguments";
        return CPOL_ERR_ARG;
    }
    const int nz = m->nz, ny = m->ny, nx = m->nx, n_vars = m->n_vars, nf = m->n_fields;
    auto bad = [&](const std::string &why) { ctx->err = "cpol_stage_model_packed: " + why; return CPOL_ERR_ARG; };
    if (n_vars < 1 || n_vars > CPOL_MAX_VARS || nz < 3 || ny < 2 || nx < 2) return bad("bad shape (need nz >= 3, ny, nx >= 2)");
    if (nf < 1 || nf > CPOL_MAX_RAW_FIELDS || m->n_load < 0 || m->n_load > CPOL_MAX_LOAD) return bad("bad field counts");
    // ---- everything is checked before anything changes
    std::vector<int> base((size_t)nf + 1, 0);
    for (int f = 0; f < nf; ++f) {
        if (m->field_levels[f] != nz && m->field_levels[f] != nz + 1) return bad("a raw field must have nz or nz + 1 levels");
        base[(size_t)f + 1] = base[(size_t)f] + m->field_levels[f];
    }
    const int total_planes = base[(size_t)nf];
    auto full = [&](int f) { return f >= 0 && f < nf && m->field_levels[f] == nz; };
    auto any = [&](int f) { return f >= 0 && f < nf; };
    if (!full(m->field_p) || !full(m->field_t) || !full(m->field_qv) || !any(m->field_hhl)) return bad("P, T, QV on nz levels and HHL are needed");
    for (int j = 0; j < m->n_load; ++j) if (!full(m->field_load[j])) return bad("a condensate field must have nz levels");
    for (int v = 0; v < n_vars; ++v) {
        const int r = m->recipe[v], f = m->source[v];
        if (r == CPOL_RECIPE_COPY || r == CPOL_RECIPE_TIMES_RHO) { if (!full(f)) return bad("COPY / TIMES_RHO need a raw field on nz levels"); }
        else if (r == CPOL_RECIPE_HALF_MEAN) { if (!any(f) || m->field_levels[f] != nz + 1) return bad("HALF_MEAN needs a raw field on nz + 1 levels"); }
        else if (r != CPOL_RECIPE_RHO && r != CPOL_RECIPE_ZEROS) return bad("unknown recipe");
    }
    if (n_planes != total_planes) return bad("the planes must cover every level of every raw field exactly once");
    const long ncell = (long)ny * nx;
    std::vector<long> out_plane((size_t)n_planes);
    std::vector<char> seen((size_t)total_planes, 0);
    for (int i = 0; i < n_planes; ++i) {
        const cpol_packed_plane &p = planes[i];
        if (!any(p.field) || p.level < 0 || p.level >= m->field_levels[p.field]) return bad("plane " + std::to_string(i) + ": field / level out of range");
        const int o = base[(size_t)p.field] + p.level;
        if (seen[(size_t)o]) return bad("plane " + std::to_string(i) + ": this (field, level) came before");
        seen[(size_t)o] = 1;
        out_plane[(size_t)i] = o;
        const char *why = packed_plane_fault(p, ncell);
        if (why) return bad("plane " + std::to_string(i) + ": " + why);
    }
    (void)hipGetLastError();            // a stale error of another user of the runtime in this thread is not ours
    if (model_on_lane(ctx, "cpol_stage_model_packed")) return CPOL_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    stencil_new_heights(ctx);           // (the levels are derived on the device: no cheap comparison, a new heights identity)
    const double t_start = wall_ms();
    const size_t plane_bytes = (size_t)nz * ncell * sizeof(float);
    const size_t h_bytes = (plane_bytes + 7) & ~(size_t)7;        // + (top, lowest level) per column behind the levels
    DevBuf arena, desc, cube;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int rc = ensure(ctx, cube, (size_t)total_planes * ncell * sizeof(float));
    if (rc == CPOL_OK) rc = upload_packed(ctx, planes, n_planes, out_plane, arena, desc);
    const double t_up = wall_ms();
    if (rc == CPOL_OK) rc = ensure(ctx, ctx->d_H, h_bytes + (size_t)ncell * sizeof(float2));
    if (rc == CPOL_OK) rc = ensure(ctx, ctx->d_V, plane_bytes * n_vars);
    if (rc == CPOL_OK) {
        DeriveArgs a{};
        a.planes = (const float *)cube.p;
        a.V = (float *)ctx->d_V.p; a.H = (float *)ctx->d_H.p; a.HT = (float2 *)((char *)ctx->d_H.p + h_bytes);
        a.ncell = ncell; a.nz = nz; a.n_vars = n_vars;
        a.base_p = base[(size_t)m->field_p]; a.base_t = base[(size_t)m->field_t]; a.base_qv = base[(size_t)m->field_qv];
        a.base_hhl = base[(size_t)m->field_hhl]; a.hhl_half = m->field_levels[m->field_hhl] == nz + 1;
        a.n_load = m->n_load;
        for (int j = 0; j < m->n_load; ++j) a.base_load[j] = base[(size_t)m->field_load[j]];
        for (int v = 0; v < n_vars; ++v) {
            a.recipe[v] = m->recipe[v];
            a.base_src[v] = (m->recipe[v] == CPOL_RECIPE_RHO || m->recipe[v] == CPOL_RECIPE_ZEROS) ? 0 : base[(size_t)m->source[v]];
        }
        a.r_d = m->r_d; a.rv_rd_m1 = m->rv_rd_m1;
        // 64 cells x kc levels x n_vars through LDS: the largest kc (a multiple of 4, <= 16) whose tile stays under 60 KB
        const bool vec4 = ((long)nz * n_vars) % 4 == 0;
        size_t lds = 0;
        for (a.kc = 16; a.kc >= 4; a.kc -= 4) {
            a.rowlen = vec4 ? a.kc * n_vars + 4 : ((a.kc * n_vars) | 1);
            lds = ((size_t)64 * a.rowlen + (size_t)64 * (a.kc + 1)) * sizeof(float);
            if (lds <= (size_t)60 * 1024) break;
        }
        for (auto &e : ev) if (hipEventCreate(&e) != hipSuccess) e = nullptr;
        if (ev[0]) (void)hipEventRecord(ev[0], ctx->stream);
        launch_unpack(ctx, arena, desc, (float *)cube.p, n_planes, ny, nx);
        if (ev[1]) (void)hipEventRecord(ev[1], ctx->stream);
        const dim3 grid((unsigned)cdiv(ncell, 64), (unsigned)cdiv(nz, a.kc));
        if (vec4) hipLaunchKernelGGL((k_model_derive<true>), grid, dim3(256), lds, ctx->stream, a);
        else hipLaunchKernelGGL((k_model_derive<false>), grid, dim3(256), lds, ctx->stream, a);
        if (ev[2]) (void)hipEventRecord(ev[2], ctx->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { ctx->err = std::string("cpol_stage_model_packed: ") + hipGetErrorString(e); rc = CPOL_ERR_HIP; }
    }
    free_buf(arena); free_buf(desc); free_buf(cube);
    if (rc == CPOL_OK) {
        float ms_unpack = 0.f, ms_derive = 0.f;
        if (ev[0] && ev[1] && ev[2]) { (void)hipEventElapsedTime(&ms_unpack, ev[0], ev[1]); (void)hipEventElapsedTime(&ms_derive, ev[1], ev[2]); }
        model_staged_tail(ctx, n_vars, nz, ny, nx, h_bytes, m->llc, m->urc, m->res, m->south_pole);
        ctx->ingest_ms[0] = t_up - t_start; ctx->ingest_ms[1] = ms_unpack; ctx->ingest_ms[2] = ms_derive;
        ctx->ingest_ms[3] = wall_ms() - t_start;
    } else if (ctx->d_H.p == nullptr || ctx->d_V.p == nullptr || rc == CPOL_ERR_HIP) {
        ctx->model_staged = false;       // the cube behind the model descriptor is gone or half written
    }
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    return rc;
}

static int n_par_of(int rule)
{
    switch (rule) {
    case CPOL_RULE_ICE_1MOM: return 3;
    case CPOL_RULE_MELTING_SNOW:
    case CPOL_RULE_MELTING_GRAUPEL: return 3;
    default: return 2;
    }
}

int cpol_set_num_hydro(cpol_ctx *ctx, int n_hydro)
{
    if (!ctx || n_hydro < 0 || n_hydro > CPOL_MAX_HYDRO) return CPOL_ERR_ARG;
    if (ctx->parent || ctx->n_children) {
        ctx->err = "cpol_set_num_hydro: not on a lane, and not while lanes of this context exist";
        return CPOL_ERR_ARG;
    }
    long total = 0;
    for (int j = 0; j < n_hydro; ++j) total += (long)ctx->hs.h[j].d.n_e * ctx->hs.h[j].d.n_t;
    if (total > 1024L * CPOL_SCAN_MAX_PER) {           // checked BEFORE any state changes
        ctx->err = "too many LUT slices (elevation x temperature bins) for the bucket scan";
        return CPOL_ERR_ARG;
    }
    ctx->hs.n_hydro = n_hydro;
    ctx->stage_serial++;
    ctx->lut_serial++;
    int base = 0;
    for (int j = 0; j < n_hydro; ++j) {
        ctx->hs.h[j].key_base = base;
        base += ctx->hs.h[j].d.n_e * ctx->hs.h[j].d.n_t;
    }
    ctx->hs.n_keys = base;
    return CPOL_OK;
}

int cpol_stage_hydro(cpol_ctx *ctx, int slot, const cpol_hydro_desc *desc, const double *table,
                     const double *pre, const double *dnu, const double *aux, int n_aux)
{
    if (!ctx || !desc || !table || slot < 0 || slot >= CPOL_MAX_HYDRO || desc->n_e < 1 ||
        desc->n_t < 1 || desc->n_d < 2) {
        if (ctx) ctx->err = "cpol_stage_hydro: bad arguments";
        return CPOL_ERR_ARG;
    }
    if (ctx->parent || ctx->n_children) {
        ctx->err = "cpol_stage_hydro: not on a lane, and not while lanes of this context exist (cpol_fork)";
        return CPOL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t tb = (size_t)desc->n_e * desc->n_t * desc->n_d * CPOL_N_SZ * sizeof(double);
    const size_t db = (size_t)desc->n_d * sizeof(double);
    int rc;
    HydroDev &h = ctx->hs.h[slot];
    const double *dev_table = nullptr;
    if (desc->table_id) {
        // the scattering table of a known identity stays resident (CPOL_ITAB_CACHE most recent):
        // a switch back to a table set seen before uploads only the small per-bin arrays
        for (auto &e : ctx->table_cache)
            if (e.id == desc->table_id && e.bytes == tb) { dev_table = (const double *)e.buf.p; e.used = ++ctx->table_clock; break; }
        if (!dev_table) {
            if (ctx->table_cache.size() >= CPOL_ITAB_CACHE) {
                // evict the least recently used entry that no staged slot points at
                size_t victim = ctx->table_cache.size();
                for (size_t k = 0; k < ctx->table_cache.size(); ++k) {
                    bool live = false;
                    for (int q = 0; q < CPOL_MAX_HYDRO; ++q)
                        live = live || (q != slot && ctx->hydro_staged[q] && ctx->hs.h[q].table == ctx->table_cache[k].buf.p);
                    if (!live && (victim == ctx->table_cache.size() || ctx->table_cache[k].used < ctx->table_cache[victim].used))
                        victim = k;
                }
                if (victim < ctx->table_cache.size()) {
                    free_buf(ctx->table_cache[victim].buf);
                    ctx->table_cache.erase(ctx->table_cache.begin() + victim);
                }
            }
            if (ctx->table_cache.size() < CPOL_ITAB_CACHE) {
                ctx->table_cache.emplace_back();
                TableCacheEntry &e = ctx->table_cache.back();
                if ((rc = upload(ctx, e.buf, table, tb)) != CPOL_OK) { ctx->table_cache.pop_back(); return rc; }
                e.id = desc->table_id; e.bytes = tb; e.used = ++ctx->table_clock;
                dev_table = (const double *)e.buf.p;
            }
        }
    }
    if (!dev_table) {
        if ((rc = upload(ctx, ctx->d_table[slot], table, tb)) != CPOL_OK) return rc;
        dev_table = (const double *)ctx->d_table[slot].p;
    }
    h.d = *desc;
    h.table = dev_table;
    h.pre = h.dnu = h.aux = nullptr;
    h.rcsw = nullptr;
    ctx->ss.s[slot] = SpecDev{};
    if (pre) {
        if ((rc = upload(ctx, ctx->d_pre[slot], pre, db)) != CPOL_OK) return rc;
        h.pre = (const double *)ctx->d_pre[slot].p;
    }
    if (dnu) {
        if ((rc = upload(ctx, ctx->d_dnu[slot], dnu, db)) != CPOL_OK) return rc;
        h.dnu = (const double *)ctx->d_dnu[slot].p;
    }
    if (aux && n_aux > 0) {
        if ((rc = upload(ctx, ctx->d_aux[slot], aux, (size_t)n_aux * sizeof(double))) != CPOL_OK)
            return rc;
        h.aux = (const double *)ctx->d_aux[slot].p;
    }
    if (desc->psd_family == CPOL_PSD_GAMMA && (!pre || !dnu)) {
        ctx->err = "cpol_stage_hydro: gamma family needs pre[] and dnu[]";
        return CPOL_ERR_ARG;
    }
    if (desc->psd_family == CPOL_PSD_GAMMA && desc->numeric_intv &&
        (desc->uniform_grid || !aux || n_aux < 3 * desc->n_d + 1)) {
        ctx->err = "cpol_stage_hydro: numeric_intv needs aux[3*n_d+1] and excludes uniform_grid";
        return CPOL_ERR_ARG;
    }
    if (desc->psd_family == CPOL_PSD_GAMMA && desc->uniform_grid &&
        (!aux || n_aux < 5 * desc->n_d + 1)) {
        ctx->err = "cpol_stage_hydro: uniform_grid needs aux[1 + 5 n_d]";
        return CPOL_ERR_ARG;
    }
    if (desc->psd_family == CPOL_PSD_MELTING && desc->tab_degree != 0 &&
        (desc->tab_degree != CPOL_MELT_DEGREE || !aux ||
         (long)n_aux < 2L * desc->n_t + (long)desc->n_t * desc->n_d * CPOL_MELT_FUNCS * (CPOL_MELT_DEGREE + 1))) {
        ctx->err = "cpol_stage_hydro: tab_degree must be 0 or CPOL_MELT_DEGREE with aux[2 n_t + n_t n_d 4 (degree+1)]";
        return CPOL_ERR_ARG;
    }
    if (desc->psd_family == CPOL_PSD_ICE_FIELD && desc->tab_degree != 0 &&
        (desc->tab_degree != CPOL_ICE_DEGREE || !desc->uniform_grid || !aux || n_aux < 12 * desc->n_d + 12 ||
         (long)n_aux < 12L * desc->n_d + 12 + (long)aux[12 * desc->n_d + 10] * CPOL_ICE_FUNCS * (CPOL_ICE_DEGREE + 1))) {
        ctx->err = "cpol_stage_hydro: ice tab_degree must be 0 or CPOL_ICE_DEGREE with the lambda-panel tables behind the recurrence block of aux[]";
        return CPOL_ERR_ARG;
    }
    if (desc->psd_family == CPOL_PSD_ICE_FIELD && (!aux || n_aux < 4 * desc->n_d + 1)) {
        ctx->err = "cpol_stage_hydro: ice family needs aux[4*n_d+1]";
        return CPOL_ERR_ARG;
    }
    h.n_par = n_par_of(desc->rule);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->hydro_staged[slot] = true;
    ctx->stage_serial++;
    ctx->lut_serial++;
    const int rc_n = cpol_set_num_hydro(ctx, slot >= ctx->hs.n_hydro ? slot + 1 : ctx->hs.n_hydro);
    if (rc_n != CPOL_OK) {
        ctx->hydro_staged[slot] = false;               // the slot does not count as staged
        return rc_n;
    }
    return CPOL_OK;
}

int cpol_stage_t_function(cpol_ctx *ctx, int which, const float *table)
{
    if (!ctx || !table || which < 0 || which >= CPOL_N_TFUN) {
        if (ctx) ctx->err = "cpol_stage_t_function: bad arguments";
        return CPOL_ERR_ARG;
    }
    if (ctx->parent || ctx->n_children) {
        ctx->err = "cpol_stage_t_function: not on a lane, and not while lanes of this context exist (cpol_fork)";
        return CPOL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = upload(ctx, ctx->d_tfun[which], table, (size_t)CPOL_TFUN_COUNT * sizeof(float))) != CPOL_OK)
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->tfun[which] = (const float *)ctx->d_tfun[which].p;
    ctx->stage_serial++;
    return CPOL_OK;
}

int cpol_prepare(cpol_ctx *ctx)
{
    if (!ctx) return CPOL_ERR_ARG;
    if (ctx->parent) return CPOL_OK;
    for (int j = 0; j < ctx->hs.n_hydro; ++j)
        if (!ctx->hydro_staged[j]) { ctx->err = "cpol_prepare: hydrometeor slot not staged"; return CPOL_ERR_ARG; }
    return build_itabs(ctx);
}

int cpol_stage_doppler_weights(cpol_ctx *ctx, int slot, const double *weights)
{
    if (!ctx || !weights || slot < 0 || slot >= CPOL_MAX_HYDRO || !ctx->hydro_staged[slot]) {
        if (ctx) ctx->err = "cpol_stage_doppler_weights: stage the hydrometeor first";
        return CPOL_ERR_ARG;
    }
    if (ctx->parent || ctx->n_children) {
        ctx->err = "cpol_stage_doppler_weights: not on a lane, and not while lanes of this context exist (cpol_fork)";
        return CPOL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const cpol_hydro_desc &d = ctx->hs.h[slot].d;
    const size_t bytes = (size_t)d.n_e * d.n_t * d.n_d * 2 * sizeof(double);
    int rc;
    if ((rc = upload(ctx, ctx->d_rcsw[slot], weights, bytes)) != CPOL_OK) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->hs.h[slot].rcsw = (const double *)ctx->d_rcsw[slot].p;
    ctx->stage_serial++;
    ctx->lut_serial++;
    return CPOL_OK;
}

int cpol_stage_spectrum_tables(cpol_ctx *ctx, int slot, const float *rcs32, const float *dgrid)
{
    if (!ctx || !rcs32 || !dgrid || slot < 0 || slot >= CPOL_MAX_HYDRO || !ctx->hydro_staged[slot]) {
        if (ctx) ctx->err = "cpol_stage_spectrum_tables: stage the hydrometeor first";
        return CPOL_ERR_ARG;
    }
    if (ctx->parent || ctx->n_children) {
        ctx->err = "cpol_stage_spectrum_tables: not on a lane, and not while lanes of this context exist (cpol_fork)";
        return CPOL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    HydroDev &h = ctx->hs.h[slot];
    // (melting species: rcs32 alone is read -- their diameter grid belongs to the gate's wet fraction, cpol_spectrum.inl)
    const size_t nr = (size_t)h.d.n_e * h.d.n_t * h.d.n_d;
    int rc;
    if ((rc = upload(ctx, ctx->d_rcs32[slot], rcs32, nr * sizeof(float))) != CPOL_OK) return rc;
    if ((rc = upload(ctx, ctx->d_dgrid[slot], dgrid, (size_t)3 * h.d.n_d * sizeof(float))) != CPOL_OK) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->ss.s[slot].rcs32 = (const float *)ctx->d_rcs32[slot].p;
    ctx->ss.s[slot].dgrid = (const float *)ctx->d_dgrid[slot].p;
    ctx->ss.s[slot].step32 = dgrid[1] - dgrid[0];
    return CPOL_OK;
}

int cpol_interp_points(cpol_ctx *ctx, int n, const float *coords, const float *heights, float *out)
{
    if (!ctx || !ctx->model_staged || n < 1 || !coords || !heights || !out) {
        if (ctx) ctx->err = "cpol_interp_points: model not staged or bad arguments";
        return CPOL_ERR_ARG;
    }
    (void)hipGetLastError();            // a stale error of another user of the runtime in this thread is not ours
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf c, h, o;
    int rc;
    if ((rc = upload(ctx, c, coords, (size_t)n * 2 * sizeof(float))) != CPOL_OK) return rc;
    if ((rc = upload(ctx, h, heights, (size_t)n * sizeof(float))) != CPOL_OK) return rc;
    const size_t ob = (size_t)n * ctx->model.n_vars * sizeof(float);
    if ((rc = ensure(ctx, o, ob)) != CPOL_OK) return rc;
    hipLaunchKernelGGL(k_interp_points, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ctx->model,
                       (const float *)c.p, (const float *)h.p, (float *)o.p, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, o.p, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    free_buf(c); free_buf(h); free_buf(o);
    return CPOL_OK;
}

// the filter kernel of the spectrum broadening: one workgroup per row, a wavefront for short rows
static void launch_broaden(const SpecBroadenArgs &ba, long n_rows, hipStream_t st)
{
    const size_t lds = (size_t)ba.n_v * sizeof(float);
    if (ba.n_v <= CPOL_BROAD_WAVE_BINS) hipLaunchKernelGGL((k_spec_broaden<64>), dim3((unsigned)n_rows), dim3(64), lds, st, ba);
    else hipLaunchKernelGGL((k_spec_broaden<256>), dim3((unsigned)n_rows), dim3(256), lds, st, ba);
}

int cpol_broaden_rows(cpol_ctx *ctx, const float *rows, int n_rows, int n_v, const double *sigma_bins, float *out)
{
    if (!ctx || !rows || !sigma_bins || !out || n_rows < 1 || n_v < 2 || n_v > 4097) {
        if (ctx) ctx->err = "cpol_broaden_rows: bad arguments (n_rows >= 1, n_v in [2, 4097])";
        return CPOL_ERR_ARG;
    }
    (void)hipGetLastError();            // a stale error of another user of the runtime in this thread is not ours
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf r, s, o;
    int rc;
    const size_t rb = (size_t)n_rows * n_v * sizeof(float);
    if ((rc = upload(ctx, r, rows, rb)) != CPOL_OK) return rc;
    if ((rc = upload(ctx, s, sigma_bins, (size_t)n_rows * sizeof(double))) != CPOL_OK) { free_buf(r); return rc; }
    if ((rc = ensure(ctx, o, rb)) != CPOL_OK) { free_buf(r); free_buf(s); return rc; }
    SpecBroadenArgs ba{};
    ba.in = (const float *)r.p; ba.out = (float *)o.p; ba.sigma = (const double *)s.p;
    ba.on = nullptr; ba.rows_per_switch = 1; ba.n_v = n_v;
    launch_broaden(ba, n_rows, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, o.p, rb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    free_buf(r); free_buf(s); free_buf(o);
    return CPOL_OK;
}

int cpol_ray_tables(const cpol_sweep_params *p, const double *az_deg, const double *el_deg,
                    const double *pts_h_deg, const double *pts_v_deg, double *traj_out,
                    double *geo_out)
{
    if (!p || !az_deg || !el_deg || !pts_h_deg || !pts_v_deg || !traj_out || !geo_out)
        return CPOL_ERR_ARG;
    const double a = 6378137.0, f = CPOL_WGS84_F, b = (1.0 - f) * a;
    for (int r = 0; r < p->n_rays; ++r) {
        for (int j = 0; j < p->n_vnodes; ++j) {
            double el = (pts_v_deg[j] + el_deg[r]) * CPOL_DEG;
            double *o = traj_out + ((long)r * p->n_vnodes + j) * 4;
            o[0] = el; o[1] = sin(el); o[2] = cos(el); o[3] = pts_v_deg[j] + el_deg[r];
        }
        for (int i = 0; i < p->n_hnodes; ++i) {
            double alpha1 = (pts_h_deg[i] + az_deg[r]) * CPOL_DEG;
            double sin_a1 = sin(alpha1), cos_a1 = cos(alpha1);
            double tan_u1 = p->sin_u1 / p->cos_u1;
            double sigma1 = atan2(tan_u1, cos_a1);
            double sin_alpha = p->cos_u1 * sin_a1;
            double cos2_alpha = 1.0 - sin_alpha * sin_alpha;
            double u2 = cos2_alpha * (a * a - b * b) / (b * b);
            double A = 1.0 + u2 / 16384.0 * (4096.0 + u2 * (-768.0 + u2 * (320.0 - 175.0 * u2)));
            double B = u2 / 1024.0 * (256.0 + u2 * (-128.0 + u2 * (74.0 - 47.0 * u2)));
            double C = f / 16.0 * cos2_alpha * (4.0 + f * (4.0 - 3.0 * cos2_alpha));
            double *o = geo_out + ((long)r * p->n_hnodes + i) * 8;
            o[0] = sin_a1; o[1] = cos_a1; o[2] = sigma1; o[3] = sin_alpha;
            o[4] = b * A; o[5] = B; o[6] = C; o[7] = alpha1;
        }
    }
    return CPOL_OK;
}

// Measurement knob (CPOL_TABLE_UPLOAD=kernel): the per-ray tables of a sweep from the page-locked staging slot (host memory
// the device can address) into the table set's device buffer by a kernel instead of hipMemcpyAsync.  It showed that the
// ~340 us the first asynchronous copy of a sweep cost in round 4's "slow mode" belong to whichever copy call comes first
// (host-to-device with the memcpy, the device-to-host copy of the results with this kernel): see report_domain_error.
__global__ __launch_bounds__(256) void k_upload_tables(uint4 *__restrict__ dst, const uint4 *__restrict__ src, long n16)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

static inline double now_ns()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e9 + (double)ts.tv_nsec;
}

static int copy_out(cpol_ctx *ctx, void *dst, const void *src, size_t bytes, bool dst_on_device)
{
    if (!dst) return CPOL_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes,
                          dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          ctx->stream));
    return CPOL_OK;
}

// The device pointers of a placement plan (cpol_place.h): the buffers of the context grown to what the plan asks for, their bases
// added.  sweep_own[i]: the buffer of array i where it is one of the sweep's own (product PLACE_SWEEP; NULL: the list has none)
static int place_resolve(cpol_ctx *ctx, const PlaceArray *arr, int n, const PlacePlan &plan, DevBuf *const *sweep_own, void **T)
{
    DevBuf *const block[PLACE_PRODUCTS] = {nullptr, &ctx->b_superob, &ctx->b_msout};
    if (plan.window) ENSURE(ctx->b_outwin, plan.win_bytes);
    for (int q = 0; q < PLACE_PRODUCTS; ++q)
        if (plan.block_bytes[q]) ENSURE(*block[q], plan.block_bytes[q]);
    for (int i = 0; i < n; ++i) {
        const PlaceWhere &w = plan.where[i];
        T[i] = nullptr;
        if (w.kind == PLACE_IN_PLACE) T[i] = (void *)arr[i].user;
        else if (w.kind == PLACE_WINDOW) T[i] = (char *)ctx->b_outwin.p + plan.win_skew + w.offset;
        else if (w.kind == PLACE_OWN && arr[i].product == PLACE_SWEEP) {
            ENSURE(*sweep_own[i], arr[i].bytes);
            T[i] = sweep_own[i]->p;
        } else if (w.kind == PLACE_OWN) T[i] = (char *)block[arr[i].product]->p + w.offset;
    }
    return CPOL_OK;
}

// ... and the copies of what neither lies in the window image (ONE copy, by the caller) nor was written in place
static int place_copy_out(cpol_ctx *ctx, const PlaceArray *arr, const PlacePlan &plan, void *const *T, bool dst_on_device)
{
    int rc;
    for (int c = 0; c < plan.n_copies; ++c) {
        const PlaceCopy &cp = plan.copies[c];
        if ((rc = copy_out(ctx, (char *)arr[cp.array].user + cp.offset, (const char *)T[cp.array] + cp.offset, cp.bytes, dst_on_device))) return rc;
    }
    return CPOL_OK;
}

// The head the product hooks share: the caller's per-gate fields, n values each, into the sweep's own output buffers, where the
// launch sequence leaves them -- the slots of `mask` that are given; slot 9 (RVEL) float64 into b_rvel, the rest float32 into b_out[k]
static int hook_upload_fields(cpol_ctx *ctx, const void *const *src, int n_slots, unsigned mask, size_t n, const void **in)
{
    int rc;
    for (int k = 0; k < n_slots; ++k) {
        if (!((mask >> k) & 1u) || !src[k]) continue;
        DevBuf &b = k == 9 ? ctx->b_rvel : ctx->b_out[k];
        if ((rc = upload(ctx, b, src[k], n * (k == 9 ? sizeof(double) : sizeof(float)))) != CPOL_OK) return rc;
        in[k] = b.p;
    }
    return CPOL_OK;
}

// ... and their tail: the plan of blocking host arrays, its device pointers, the hook's launch(T), the copies, the wait
extern "C++" {
template <int N, class Launch>
static int hook_finish(cpol_ctx *ctx, const PlaceArray (&arr)[N], DevBuf *const *own, Launch launch)
{
    PlacePlan plan;
    place_outputs(arr, N, 0, false, &plan);
    void *T[N];
    int rc;
    if ((rc = place_resolve(ctx, arr, N, plan, own, T)) != CPOL_OK) return rc;
    if ((rc = launch(T)) != CPOL_OK) return rc;
    if ((rc = place_copy_out(ctx, arr, plan, T, false)) != CPOL_OK) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return CPOL_OK;
}
}

// ---- superobservations (cpol_superob, cpol_superob.inl): the checks and the launch, shared by the launch sequence and the test hook ----
enum { SO_RVEL = CPOL_SUPEROB_RVEL, SO_COUNT = CPOL_SUPEROB_FIELDS, SO_N };
struct SuperobPlan {
    long cells;
    int rpb, wr, wc;
};

// every refusal of a cpol_superob for a call of n_rows rows (rays_default: what rays_per_block = 0 means); queues nothing.
// arr[SO_N]: the caller's arrays for the placement plan (cpol_place.h): ten fields, then count
static int superob_plan(cpol_ctx *ctx, const cpol_superob *so, int n_rows, int rays_default, int ng, bool doppler, SuperobPlan *pl,
                        PlaceArray *arr)
{
    auto bad = [&](const char *why) { ctx->err = std::string("cpol_superob: ") + why; return CPOL_ERR_ARG; };
    if (so->ray_window < 1 || so->gate_window < 1) return bad("ray_window and gate_window must be >= 1");
    if ((long)so->ray_window * so->gate_window > 65535) return bad("ray_window * gate_window must be <= 65535 (count is uint16)");
    if (!(so->min_valid_fraction > 0.0 && so->min_valid_fraction <= 1.0)) return bad("min_valid_fraction must lie in (0, 1]");
    pl->rpb = so->rays_per_block ? so->rays_per_block : rays_default;
    if (so->rays_per_block < 0 || n_rows % pl->rpb != 0) return bad("rays_per_block must be >= 0 and divide the rows of the call");
    void *const f[SO_N] = {so->ZH, so->ZV, so->ZDR, so->KDP, so->DELTA_HV, so->PHIDP, so->RHOHV, so->ATT_H, so->ATT_V, so->RVEL,
                           so->count};
    pl->wr = cdiv(pl->rpb, so->ray_window);
    pl->wc = cdiv(ng, so->gate_window);
    pl->cells = (long)(n_rows / pl->rpb) * pl->wr * pl->wc;
    bool any = false;
    for (int k = 0; k < SO_N; ++k) {
        arr[k] = PlaceArray{};
        arr[k].user = (uintptr_t)f[k];
        arr[k].bytes = (size_t)pl->cells * (k == SO_RVEL ? sizeof(double) : k == SO_COUNT ? CPOL_SUPEROB_FIELDS * sizeof(uint16_t) : sizeof(float));
        arr[k].produced = true;
        arr[k].product = PLACE_SUPEROB;
        any = any || (f[k] && k != SO_COUNT);
    }
    arr[SO_COUNT].rows = CPOL_SUPEROB_FIELDS;           // (count: the rows of requested fields alone are the caller's to be written)
    for (int k = 0; k < SO_COUNT; ++k)
        if (f[k]) arr[SO_COUNT].row_mask |= 1u << k;
    if (!any) return bad("no output pointer set");
    if (so->RVEL && !doppler) return bad("RVEL needs simulate_doppler");
    return CPOL_OK;
}

// in: the per-gate device arrays in the order of `count`'s rows (slot ZDR unused, slot RVEL float64); T: where the kernel writes
static int superob_launch(cpol_ctx *ctx, const cpol_superob *so, const SuperobPlan &pl, const void *const in[CPOL_SUPEROB_FIELDS],
                          void *const T[SO_N], int ng, bool zero_rest, hipStream_t st)
{
    SuperobArgs sa{};
    for (int k = 0; k < CPOL_SUPEROB_FIELDS; ++k) {
        sa.in[k] = (k == SO_RVEL || k == CPOL_SUPEROB_ZDR) ? nullptr : (const float *)in[k];
        sa.out[k] = k == SO_RVEL ? nullptr : (float *)T[k];
        if (T[k]) sa.field[sa.n_fields++] = k;
    }
    sa.in_rvel = (const double *)in[SO_RVEL];
    sa.out_rvel = (double *)T[SO_RVEL];
    sa.count = (unsigned short *)T[SO_COUNT];
    sa.n_cells = pl.cells;
    sa.min_valid_fraction = so->min_valid_fraction;
    sa.n_gates = ng; sa.R = so->ray_window; sa.G = so->gate_window;
    sa.rays_per_block = pl.rpb; sa.win_rows = pl.wr; sa.win_cols = pl.wc;
    sa.zero_rest = zero_rest;
    hipLaunchKernelGGL(k_superob, dim3(cdiv(pl.cells, 256), sa.n_fields), dim3(256), 0, st, sa);
    HIPCHK(hipGetLastError());
    return CPOL_OK;
}

// The test hook cpol_debug_read "superob_fields": k_superob on caller-supplied per-gate arrays (host memory in, host memory out,
// blocking) -- the kernel on inputs no sweep produces (ZV missing where ZH is not, infinities, signed zeros, the largest window).
struct SuperobHook {
    int32_t n_rows, n_gates;
    const void *in[CPOL_SUPEROB_FIELDS];    // [n_rows * n_gates] float32 (slot ZDR unused; slot RVEL float64); NULL = not given
    cpol_superob so;                        // rays_per_block = 0: n_rows; a requested field needs its input (ZDR: ZH and ZV)
};

static int superob_hook(cpol_ctx *ctx, const SuperobHook *h)
{
    if (h->n_rows < 1 || h->n_gates < 1 || (long)h->n_rows * h->n_gates >= (1L << 31)) { ctx->err = "superob_fields: bad shape"; return CPOL_ERR_ARG; }
    SuperobPlan pl{};
    PlaceArray arr[SO_N];
    int rc = superob_plan(ctx, &h->so, h->n_rows, h->n_rows, h->n_gates, true, &pl, arr);
    if (rc != CPOL_OK) return rc;
    for (int k = 0; k < CPOL_SUPEROB_FIELDS; ++k) {
        const bool need = k == CPOL_SUPEROB_ZDR ? false : (arr[k].user || (arr[CPOL_SUPEROB_ZDR].user && k <= CPOL_SUPEROB_ZV));
        if (need && !h->in[k]) { ctx->err = "superob_fields: a requested field has no input"; return CPOL_ERR_ARG; }
    }
    HIPCHK(hipSetDevice(ctx->device));
    const void *in[CPOL_SUPEROB_FIELDS] = {};
    if ((rc = hook_upload_fields(ctx, h->in, CPOL_SUPEROB_FIELDS, ~(1u << CPOL_SUPEROB_ZDR), (size_t)h->n_rows * h->n_gates, in)) != CPOL_OK) return rc;
    return hook_finish(ctx, arr, nullptr, [&](void *const *T) { return superob_launch(ctx, &h->so, pl, in, T, h->n_gates, false, ctx->stream); });
}

// ---- ensemble statistics (cpol_member_stats, cpol_member_stats.inl): the checks, the pass and the launches, shared by the
// launch sequence and the test hook ----
enum { MS_MEAN = 0, MS_SPREAD = CPOL_MS_FIELDS, MS_MIN = 2 * CPOL_MS_FIELDS, MS_MAX = 3 * CPOL_MS_FIELDS, MS_COUNT = 4 * CPOL_MS_FIELDS,
       MS_EXCEED, MS_QUANTILE = MS_EXCEED + CPOL_MS_FIELDS, MS_BELOW = MS_QUANTILE + CPOL_MS_FIELDS, MS_EQUAL = MS_BELOW + CPOL_MS_FIELDS,
       MS_CRPS = MS_EQUAL + CPOL_MS_FIELDS, MS_N = MS_CRPS + CPOL_MS_FIELDS };
struct MemberStatsPlan {
    long cells;
    int n_sets;
    bool begin, finish;
    int n_thr[CPOL_MS_FIELDS];
    double thr[CPOL_MS_FIELDS][CPOL_MS_MAX_THR];    // as the kernels compare them (float32 fields: rounded once)
    bool q_any;                                     // a folded field has quantiles
    int n_q[CPOL_MS_FIELDS];
    double q[CPOL_MS_FIELDS][CPOL_MS_MAX_Q];
    bool v_on;                                      // the call carries a cpol_member_verify
    unsigned v_fields;
    int v_fair;
};

// every refusal of a cpol_member_stats, and of the cpol_member_verify beside it (mv; NULL: none), for a call that folds n_sets row
// sets of n_cells cells; queues and changes nothing.
// arr[MS_N]: a finishing call's arrays for the placement plan (cpol_place.h): the caller's pointers, folded fields only
static int member_stats_plan(cpol_ctx *ctx, const cpol_member_stats *ms, const cpol_member_verify *mv, long n_cells, int n_sets, bool doppler,
                             MemberStatsPlan *pl, PlaceArray *arr)
{
    auto bad = [&](const char *why) { ctx->err = std::string("cpol_member_stats: ") + why; return CPOL_ERR_ARG; };
    auto bad_v = [&](const char *why) { ctx->err = std::string("cpol_member_verify: ") + why; return CPOL_ERR_ARG; };
    const cpol_ctx::MemberPass &ps = ctx->mpass;
    if (ms->phase < 0 || ms->phase > 3) return bad("phase must lie in 0..3 (bit 0: begin, bit 1: finish)");
    if (ms->min_members < 1) return bad("min_members must be >= 1");
    if (ms->fields == 0 || (ms->fields >> CPOL_MS_FIELDS) != 0) return bad("fields: a mask over the ten fields, at least one");
    if (((ms->fields >> CPOL_MS_RVEL) & 1u) && !doppler) return bad("RVEL needs simulate_doppler");
    if (n_cells < 1 || n_cells >= (1L << 31)) return bad("n_cells must lie in [1, 2^31)");
    *pl = MemberStatsPlan{};
    for (int k = 0; k < MS_N; ++k) { arr[k] = PlaceArray{}; arr[k].product = PLACE_STATS; }
    pl->cells = n_cells;
    pl->n_sets = n_sets;
    pl->begin = (ms->phase & 1) != 0;
    pl->finish = (ms->phase & 2) != 0;
    for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
        const int nt = ms->n_thresholds[k];
        if (nt < 0 || nt > CPOL_MS_MAX_THR) return bad("n_thresholds must lie in 0..8");
        if (!((ms->fields >> k) & 1u)) continue;          // (the thresholds of a field that is not folded are not read)
        if (nt > 0 && !ms->thresholds[k]) return bad("n_thresholds > 0 needs the thresholds");
        pl->n_thr[k] = nt;
        for (int t = 0; t < nt; ++t) {
            const double v = ms->thresholds[k][t];
            if (v != v) return bad("a threshold is NaN");
            pl->thr[k][t] = k == CPOL_MS_RVEL ? v : (double)(float)v;
        }
    }
    if (ms->quantile_method < 0 || ms->quantile_method > 3) return bad("quantile_method must lie in 0..3 (linear, lower, higher, nearest)");
    if (ms->quantile_capacity < 0 || ms->quantile_capacity > CPOL_MS_MAX_Q_MEMBERS) return bad("quantile_capacity must lie in 0..128");
    for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
        const int nq = ms->n_quantiles[k];
        if (nq < 0 || nq > CPOL_MS_MAX_Q) return bad("n_quantiles must lie in 0..8");
        if (!((ms->fields >> k) & 1u) || nq == 0) continue;   // (the quantile lists of a field that is not folded are not read)
        if (!ms->quantiles[k]) return bad("n_quantiles > 0 needs the quantiles");
        if (ms->quantile_capacity == 0) return bad("quantiles need quantile_capacity >= 1");
        pl->n_q[k] = nq;
        pl->q_any = true;
        for (int t = 0; t < nq; ++t) {
            const double v = ms->quantiles[k][t];
            if (!(v >= 0.0 && v <= 1.0)) return bad("a quantile is NaN or outside [0, 1]");
            pl->q[k][t] = v;
        }
    }
    if (mv) {
        if (mv->fields == 0 || (mv->fields >> CPOL_MS_FIELDS) != 0) return bad_v("fields: a mask over the ten fields, at least one");
        if (mv->fields & ~ms->fields) return bad_v("a verified field is not among the folded fields (member_stats->fields)");
        if (mv->fair != 0 && mv->fair != 1) return bad_v("fair must be 0 or 1");
        if (ms->quantile_capacity == 0) return bad_v("a verified field keeps its members: member_stats->quantile_capacity >= 1");
        pl->v_on = true; pl->v_fields = mv->fields; pl->v_fair = mv->fair;
    }
    if (!pl->begin) {
        if (!ps.open) return bad("no pass is open: the first call of a pass carries the begin bit");
        bool same = ps.n_cells == n_cells && ps.fields == ms->fields && ps.min_members == ms->min_members;
        for (int k = 0; k < CPOL_MS_FIELDS && same; ++k) {
            same = ps.n_thr[k] == pl->n_thr[k];
            for (int t = 0; t < pl->n_thr[k] && same; ++t) same = ps.thr[k][t] == pl->thr[k][t];
        }
        if (!same) return bad("n_cells, fields, thresholds or min_members differ from the open pass");
        same = ps.q_capacity == ms->quantile_capacity && ps.q_method == ms->quantile_method;
        for (int k = 0; k < CPOL_MS_FIELDS && same; ++k) {
            same = ps.n_q[k] == pl->n_q[k];
            for (int t = 0; t < pl->n_q[k] && same; ++t) same = ps.q[k][t] == pl->q[k][t];
        }
        if (!same) return bad("quantile_capacity, quantile_method or the quantiles differ from the open pass");
        if (pl->v_on && !ps.v_on) return bad_v("the open pass was begun without the struct");
        if (!pl->v_on && ps.v_on) return bad_v("the open pass was begun with the struct: every call of the pass carries it");
        if (pl->v_on && (ps.v_fields != pl->v_fields || ps.v_fair != pl->v_fair)) return bad_v("fields or fair differ from the open pass");
    }
    if ((pl->q_any || pl->v_on) && (pl->begin ? 0 : ps.folded) + n_sets > ms->quantile_capacity)
        return bad("more members than quantile_capacity in a pass with quantiles or a verification");
    if ((pl->begin ? 0 : ps.folded) + n_sets > 65535) return bad("more than 65535 members in a pass (the counts are uint16)");
    if (pl->finish) {
        bool any = false;
        const auto asked = [&](int i, void *user, size_t bytes) { arr[i].user = (uintptr_t)user; arr[i].bytes = bytes; arr[i].produced = true; };
        for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
            if (!((ms->fields >> k) & 1u)) continue;
            const size_t w = k == CPOL_MS_RVEL ? sizeof(double) : sizeof(float);
            void *const f[4] = {ms->mean[k], ms->spread[k], ms->min[k], ms->max[k]};
            for (int a = 0; a < 4; ++a) asked(a * CPOL_MS_FIELDS + k, f[a], (size_t)n_cells * w);
            if (pl->n_thr[k] > 0) asked(MS_EXCEED + k, ms->exceed[k], (size_t)pl->n_thr[k] * n_cells * sizeof(uint16_t));
            if (pl->n_q[k] > 0) asked(MS_QUANTILE + k, ms->quantile[k], (size_t)pl->n_q[k] * n_cells * w);
        }
        asked(MS_COUNT, ms->count, (size_t)CPOL_MS_FIELDS * n_cells * sizeof(uint16_t));
        arr[MS_COUNT].rows = CPOL_MS_FIELDS;            // (count: the rows of folded fields alone are the caller's to be written)
        arr[MS_COUNT].row_mask = ms->fields;
        for (int k = 0; k < CPOL_MS_FIELDS && pl->v_on; ++k) {
            if (!((pl->v_fields >> k) & 1u)) continue;
            if (!mv->obs[k]) return bad_v("a finishing call needs the observations (obs) of every verified field");
            if (!mv->below[k] && !mv->equal[k] && !mv->crps[k]) return bad_v("a finishing call needs an output pointer for every verified field");
            asked(MS_BELOW + k, mv->below[k], (size_t)n_cells * sizeof(uint16_t));
            asked(MS_EQUAL + k, mv->equal[k], (size_t)n_cells * sizeof(uint16_t));
            asked(MS_CRPS + k, mv->crps[k], (size_t)n_cells * (k == CPOL_MS_RVEL ? sizeof(double) : sizeof(float)));
        }
        for (int k = 0; k < MS_N; ++k) any = any || arr[k].user;
        if (!any) return bad("a finishing call needs an output pointer");
    }
    return CPOL_OK;
}

// The pass (begun here, when the call carries the begin bit: the state block is sized and the pass's terms are noted), the fold
// of the call's row sets and, for a finishing call, the outputs.  in: the per-gate device arrays in the order of `count`'s rows
// (slot RVEL float64), row set m at element m * cells; T: where k_member_finish writes.
// mv (NULL: none): the verification of a finishing call, its observations host arrays (obs_on_host: copied to b_mvobs on `st`
// first) or arrays the device reads in place.
static int member_stats_launch(cpol_ctx *ctx, const cpol_member_stats *ms, const MemberStatsPlan &pl, const void *const in[CPOL_MS_FIELDS],
                               void *const T[MS_N], bool zero_rest, hipStream_t st, const cpol_member_verify *mv = nullptr,
                               bool obs_on_host = false)
{
    cpol_ctx::MemberPass &ps = ctx->mpass;
    if (pl.begin) {
        const size_t a2 = ((size_t)pl.cells * sizeof(uint16_t) + 255) & ~(size_t)255, a4 = ((size_t)pl.cells * sizeof(float) + 255) & ~(size_t)255;
        const size_t a8 = ((size_t)pl.cells * sizeof(double) + 255) & ~(size_t)255;
        size_t total = 0;
        for (int k = 0; k < CPOL_MS_FIELDS; ++k)
            if ((ms->fields >> k) & 1u) total += a2 + 2 * a8 + 2 * (k == CPOL_MS_RVEL ? a8 : a4) + (size_t)pl.n_thr[k] * a2;
        size_t stash_total = 0;                               // the members of the fields with quantiles: [capacity][cells] each
        for (int k = 0; k < CPOL_MS_FIELDS; ++k)
            if (pl.n_q[k] > 0 || ((pl.v_fields >> k) & 1u)) stash_total += ((size_t)ms->quantile_capacity * pl.cells * (k == CPOL_MS_RVEL ? sizeof(double) : sizeof(float)) + 255) & ~(size_t)255;
        ps.open = false;                                      // (a begin that fails below leaves no pass behind)
        ENSURE(ctx->b_mstate, total);
        if (stash_total) ENSURE(ctx->b_mstash, stash_total);
        char *qs = (char *)ctx->b_mstash.p;
        for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
            ps.stash[k] = nullptr;
            if (pl.n_q[k] == 0 && !((pl.v_fields >> k) & 1u)) continue;
            ps.stash[k] = qs;
            qs += ((size_t)ms->quantile_capacity * pl.cells * (k == CPOL_MS_RVEL ? sizeof(double) : sizeof(float)) + 255) & ~(size_t)255;
        }
        ps.q_capacity = ms->quantile_capacity; ps.q_method = ms->quantile_method; ps.q_any = pl.q_any;
        memcpy(ps.n_q, pl.n_q, sizeof ps.n_q);
        memcpy(ps.q, pl.q, sizeof ps.q);
        ps.v_on = pl.v_on; ps.v_fields = pl.v_fields; ps.v_fair = pl.v_fair;
        char *q = (char *)ctx->b_mstate.p;
        for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
            ps.st[k] = MemberState{};
            if (!((ms->fields >> k) & 1u)) continue;
            ps.st[k].n = (unsigned short *)q; q += a2;
            ps.st[k].mean = (double *)q;      q += a8;
            ps.st[k].m2 = (double *)q;        q += a8;
            ps.st[k].lo = q;                  q += k == CPOL_MS_RVEL ? a8 : a4;
            ps.st[k].hi = q;                  q += k == CPOL_MS_RVEL ? a8 : a4;
            ps.st[k].k = (unsigned short *)q; q += (size_t)pl.n_thr[k] * a2;      // (indexed [t][n_cells]: rows n_cells elements apart)
        }
        ps.n_cells = pl.cells; ps.fields = ms->fields; ps.min_members = ms->min_members; ps.folded = 0;
        memcpy(ps.n_thr, pl.n_thr, sizeof ps.n_thr);
        memcpy(ps.thr, pl.thr, sizeof ps.thr);
        ps.open = true;
    }
    MemberStatsArgs a{};
    for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
        if (!((ps.fields >> k) & 1u)) continue;
        a.field[a.n_fields++] = k;
        a.in[k] = in[k];
        a.st[k] = ps.st[k];
        a.n_thr[k] = ps.n_thr[k];
        a.stash[k] = ps.stash[k];
    }
    a.row0 = (int)ps.folded;
    memcpy(a.thr, ps.thr, sizeof a.thr);
    a.n_sets = pl.n_sets; a.begin = pl.begin; a.need = ps.min_members; a.n_cells = pl.cells;
    const dim3 grid(cdiv(pl.cells, 256), a.n_fields);
    if (pl.n_sets > 0 || pl.begin) {
        hipLaunchKernelGGL(k_member_fold, grid, dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        ps.folded += pl.n_sets;
    }
    if (pl.finish) {
        for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
            a.o_mean[k] = T[MS_MEAN + k]; a.o_spread[k] = T[MS_SPREAD + k]; a.o_min[k] = T[MS_MIN + k]; a.o_max[k] = T[MS_MAX + k];
            a.o_exceed[k] = (unsigned short *)T[MS_EXCEED + k];
        }
        a.o_count = (unsigned short *)T[MS_COUNT];
        a.zero_rest = zero_rest;
        hipLaunchKernelGGL(k_member_finish, grid, dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        // the quantiles of the fields that have them and whose output is wanted: one wavefront per 64 cells, each lane's counting
        // members sorted in its own LDS column (members x 64 keys of the widest field: <= 32 KiB, with RVEL <= 64 KiB)
        MemberQuantileArgs qa{};
        int n_qf = 0;
        size_t key_bytes = sizeof(float);
        for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
            if (ps.n_q[k] == 0 || !ps.stash[k] || !T[MS_QUANTILE + k]) continue;
            qa.field[n_qf++] = k;
            qa.stash[k] = ps.stash[k];
            qa.out[k] = T[MS_QUANTILE + k];
            qa.n_q[k] = ps.n_q[k];
            if (k == CPOL_MS_RVEL) key_bytes = sizeof(double);
        }
        if (n_qf > 0) {                                       // (member_stats_plan: folded <= quantile_capacity <= 128)
            memcpy(qa.q, ps.q, sizeof qa.q);
            qa.members = (int)ps.folded; qa.method = ps.q_method; qa.need = ps.min_members; qa.n_cells = pl.cells;
            hipLaunchKernelGGL(k_member_quantile, dim3(cdiv(pl.cells, 64), n_qf), dim3(64), (size_t)ps.folded * 64 * key_bytes, st, qa);
            HIPCHK(hipGetLastError());
        }
        // the verification of the fields that have one and whose output is wanted: the same column, sorted once more, read
        // against the observation (member_stats_plan: folded <= quantile_capacity <= 128; obs is there for every verified field)
        if (mv && ps.v_on) {
            MemberVerifyArgs va{};
            int n_vf = 0;
            size_t vkey_bytes = sizeof(float), obs_total = 0;
            const size_t a4 = ((size_t)pl.cells * sizeof(float) + 255) & ~(size_t)255, a8 = ((size_t)pl.cells * sizeof(double) + 255) & ~(size_t)255;
            for (int k = 0; k < CPOL_MS_FIELDS; ++k) {
                if (!((ps.v_fields >> k) & 1u) || !ps.stash[k]) continue;
                if (!T[MS_BELOW + k] && !T[MS_EQUAL + k] && !T[MS_CRPS + k]) continue;
                va.field[n_vf++] = k;
                va.stash[k] = ps.stash[k];
                va.obs[k] = mv->obs[k];
                va.below[k] = (unsigned short *)T[MS_BELOW + k]; va.equal[k] = (unsigned short *)T[MS_EQUAL + k]; va.crps[k] = T[MS_CRPS + k];
                if (k == CPOL_MS_RVEL) vkey_bytes = sizeof(double);
                obs_total += k == CPOL_MS_RVEL ? a8 : a4;
            }
            if (n_vf > 0 && obs_on_host) {
                ENSURE(ctx->b_mvobs, obs_total);
                char *o = (char *)ctx->b_mvobs.p;
                for (int j = 0; j < n_vf; ++j) {
                    const int k = va.field[j];
                    HIPCHK(hipMemcpyAsync(o, mv->obs[k], (size_t)pl.cells * (k == CPOL_MS_RVEL ? sizeof(double) : sizeof(float)), hipMemcpyHostToDevice, st));
                    va.obs[k] = o;
                    o += k == CPOL_MS_RVEL ? a8 : a4;
                }
            }
            if (n_vf > 0) {
                va.members = (int)ps.folded; va.fair = ps.v_fair; va.need = ps.min_members; va.n_cells = pl.cells;
                hipLaunchKernelGGL(k_member_verify, dim3(cdiv(pl.cells, 64), n_vf), dim3(64), (size_t)ps.folded * 64 * vkey_bytes, st, va);
                HIPCHK(hipGetLastError());
            }
        }
        ps.open = false;
    }
    return CPOL_OK;
}

// The test hook cpol_debug_read "member_stats_fields": the product's fold and finish on caller-supplied members (host memory
// in, host memory out, blocking), phase by phase -- the kernels on inputs no sweep produces and on passes cut at will.
struct MemberStatsHook {
    int32_t n_members;
    int64_t n_cells;
    const void *in[CPOL_MS_FIELDS];         // [n_members][n_cells] float32 (slot RVEL float64)
    cpol_member_stats ms;
};

// ... and "member_verify_fields": the same with a verification beside it (host observations and outputs)
struct MemberVerifyHook {
    int32_t n_members;
    int64_t n_cells;
    const void *in[CPOL_MS_FIELDS];
    cpol_member_stats ms;
    cpol_member_verify mv;
};
static_assert(offsetof(MemberVerifyHook, ms) == offsetof(MemberStatsHook, ms), "the two hooks share their head");

static int member_stats_hook(cpol_ctx *ctx, const MemberStatsHook *h, const cpol_member_verify *mv = nullptr)
{
    if (h->n_members < 0 || h->n_cells < 1 || h->n_cells >= (1L << 31) || (long)h->n_members * h->n_cells >= (1L << 31)) {
        ctx->err = "member_stats_fields: bad shape";
        return CPOL_ERR_ARG;
    }
    MemberStatsPlan pl{};
    PlaceArray arr[MS_N];
    int rc = member_stats_plan(ctx, &h->ms, mv, (long)h->n_cells, h->n_members, true, &pl, arr);
    if (rc != CPOL_OK) return rc;
    for (int k = 0; k < CPOL_MS_FIELDS; ++k)
        if (((h->ms.fields >> k) & 1u) && h->n_members > 0 && !h->in[k]) { ctx->err = "member_stats_fields: a folded field has no input"; return CPOL_ERR_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)h->n_members * (size_t)h->n_cells;
    const void *in[CPOL_MS_FIELDS] = {};
    if ((rc = hook_upload_fields(ctx, h->in, CPOL_MS_FIELDS, n > 0 ? h->ms.fields : 0u, n, in)) != CPOL_OK) return rc;
    return hook_finish(ctx, arr, nullptr, [&](void *const *T) { return member_stats_launch(ctx, &h->ms, pl, in, T, false, ctx->stream, mv, true); });
}

// ---- spectrum moments (cpol_spectrum_moments, k_spec_moments in cpol_spectrum.inl): the checks and the launch, shared by the
// launch sequence and the test hook ----
enum { SM_MOMENTS = 0, SM_COUNT, SM_N };

// every refusal of a cpol_spectrum_moments for a call of n_rg gates; queues nothing.  arr[SM_N]: the caller's arrays for the
// placement plan (cpol_place.h): arrays of the sweep itself, each with a grow-only buffer of its own
static int spec_moments_plan(cpol_ctx *ctx, const cpol_spectrum_moments *sm, long n_rg, bool dop3, PlaceArray *arr)
{
    auto bad = [&](const char *why) { ctx->err = std::string("cpol_spectrum_moments: ") + why; return CPOL_ERR_ARG; };
    if (!dop3) return bad("the moments are those of the Doppler spectrum: simulate_doppler must be 3");
    if (sm->fields == 0 || (sm->fields >> CPOL_SM_FIELDS) != 0) return bad("fields must name at least one of the 8 rows and no other bit");
    if (sm->min_bins < 1 || sm->min_bins > 65535) return bad("min_bins must lie in 1 ... 65535");
    if (!(sm->min_power >= 0.0 && sm->min_power <= 1.7976931348623157e308)) return bad("min_power must be >= 0 and finite");
    if (!sm->moments) return bad("moments is NULL");
    arr[SM_MOMENTS] = PlaceArray{};
    arr[SM_MOMENTS].user = (uintptr_t)sm->moments;
    arr[SM_MOMENTS].bytes = (size_t)CPOL_SM_FIELDS * n_rg * sizeof(double);
    arr[SM_MOMENTS].rows = CPOL_SM_FIELDS;              // (only the rows in `fields` are the caller's to be written)
    arr[SM_MOMENTS].row_mask = sm->fields;
    arr[SM_COUNT] = PlaceArray{};
    arr[SM_COUNT].user = (uintptr_t)sm->count;
    arr[SM_COUNT].bytes = (size_t)n_rg * sizeof(uint16_t);
    arr[SM_MOMENTS].produced = arr[SM_COUNT].produced = true;
    arr[SM_MOMENTS].product = arr[SM_COUNT].product = PLACE_SWEEP;
    return CPOL_OK;
}

// spectrum [n_rg][n_v] and varray [n_v]: device arrays; T: where the kernel writes
static int spec_moments_launch(cpol_ctx *ctx, const cpol_spectrum_moments *sm, const double *spectrum, const double *varray,
                               void *const T[SM_N], long n_rg, int n_v, bool zero_rest, hipStream_t st)
{
    SpecMomentsArgs ma{};
    ma.spectrum = spectrum; ma.varray = varray;
    ma.moments = (double *)T[SM_MOMENTS];
    ma.count = (unsigned short *)T[SM_COUNT];
    ma.n_rg = n_rg; ma.n_v = n_v;
    ma.fields = sm->fields; ma.min_bins = sm->min_bins; ma.min_power = sm->min_power;
    ma.zero_rest = zero_rest;
    hipLaunchKernelGGL(k_spec_moments, dim3((unsigned)cdiv(n_rg, CPOL_SM_GATES_PER_BLOCK)), dim3(64 * CPOL_SM_GATES_PER_BLOCK), 0, st, ma);
    HIPCHK(hipGetLastError());
    return CPOL_OK;
}

// The test hook cpol_debug_read "spectrum_moments_rows": k_spec_moments on caller-supplied spectra (host memory in, host memory
// out, blocking) -- the kernel on rows no sweep produces (every row length, infinities, subnormals, ties, rows without a bin).
struct SpecMomentsHook {
    int32_t n_rows, n_v;
    const double *spectrum;                 // [n_rows][n_v]: every row a gate
    const double *varray;                   // [n_v]
    cpol_spectrum_moments sm;               // host output pointers sized for n_rows gates
};

static int spec_moments_hook(cpol_ctx *ctx, const SpecMomentsHook *h)
{
    if (h->n_rows < 1 || h->n_v < 1 || h->n_v > 4097 || !h->spectrum || !h->varray) {
        ctx->err = "spectrum_moments_rows: bad shape (n_rows >= 1, n_v in 1 ... 4097) or a NULL input";
        return CPOL_ERR_ARG;
    }
    PlaceArray arr[SM_N];
    int rc = spec_moments_plan(ctx, &h->sm, h->n_rows, true, arr);
    if (rc != CPOL_OK) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = upload(ctx, ctx->b_spectrum, h->spectrum, (size_t)h->n_rows * h->n_v * sizeof(double))) != CPOL_OK) return rc;
    if ((rc = upload(ctx, ctx->b_smvar, h->varray, (size_t)h->n_v * sizeof(double))) != CPOL_OK) return rc;
    DevBuf *const own[SM_N] = {&ctx->b_smom, &ctx->b_smcount};
    return hook_finish(ctx, arr, own, [&](void *const *T) {
        return spec_moments_launch(ctx, &h->sm, (const double *)ctx->b_spectrum.p, (const double *)ctx->b_smvar.p, T, h->n_rows, h->n_v, false, ctx->stream);
    });
}

// ---- sweep histograms (cpol_histogram, k_hist in cpol_hist.inl): the checks (cpol_hist.h), the pass and the launches, shared by
// the launch sequence and the test hook ----
// every refusal of a cpol_histogram for the call `c`; queues nothing and leaves the pass as it is.  arr[CPOL_HIST_FIELDS]: the
// caller's counts for the placement plan (cpol_place.h): arrays of the sweep itself, each with a grow-only buffer of its own,
// produced by a finishing call alone
static int hist_plan(cpol_ctx *ctx, const cpol_histogram *h, const HistCall &c, HistPlan *pl, PlaceArray *arr)
{
    const char *why = nullptr;
    try {
        why = hist_check(h, c, ctx->hpass, pl);
    } catch (...) {
        ctx->err = "cpol_histogram: out of host memory";
        return CPOL_ERR_NOMEM;
    }
    if (why) { ctx->err = std::string("cpol_histogram: ") + why; return CPOL_ERR_ARG; }
    for (int k = 0; k < CPOL_HIST_FIELDS; ++k) {
        arr[k] = PlaceArray{};
        if (!pl->finish || !pl->cells[k]) continue;
        arr[k].user = (uintptr_t)h->counts[k];
        arr[k].bytes = (size_t)pl->n_blocks * pl->cells[k] * sizeof(uint64_t);
        arr[k].produced = true;
        arr[k].product = PLACE_SWEEP;
    }
    return CPOL_OK;
}

// in: the per-gate device arrays in the order of the fields (slot RVEL float64); y: the ordinate's device array, holding y_gates
// gates; n_rg: the gates of the call; T: where a finishing call's counts go.  Begins, counts, finishes; then the pass is advanced
static int hist_launch(cpol_ctx *ctx, const cpol_histogram *h, const HistPlan &pl, const void *const in[CPOL_HIST_FIELDS], const void *y,
                       long y_gates, long n_rg, int ng, void *const T[CPOL_HIST_FIELDS], hipStream_t st)
{
    // the edges of the pass on the device: per requested field its abscissa's, then the ordinate's, each at a multiple of 8 bytes
    size_t e_off[CPOL_HIST_FIELDS] = {}, e_y = 0, e_bytes = 0;
    for (int i = 0; i < pl.n_fields; ++i) {
        const int k = pl.field[i];
        e_off[k] = e_bytes;
        e_bytes += ((size_t)pl.n_ex[k] * (hist_field_type(k) == HIST_T_F64 ? 8 : 4) + 7) & ~(size_t)7;
    }
    e_y = e_bytes;
    e_bytes += ((size_t)pl.n_ey * 8 + 7) & ~(size_t)7;
    if (pl.begin) {
        std::vector<char> &blob = ctx->hedges_host;     // (kept by the context: it outlives the copy whatever the runtime does)
        try { blob.assign(e_bytes, 0); } catch (...) { ctx->err = "cpol_histogram: out of host memory"; return CPOL_ERR_NOMEM; }
        const auto put = [&](size_t off, const std::vector<double> &e, int type) {
            for (size_t j = 0; j < e.size(); ++j) {
                if (type == HIST_T_F64) memcpy(blob.data() + off + 8 * j, &e[j], 8);
                else { const float f = (float)e[j]; memcpy(blob.data() + off + 4 * j, &f, 4); }
            }
        };
        for (int i = 0; i < pl.n_fields; ++i) put(e_off[pl.field[i]], pl.ex[pl.field[i]], hist_field_type(pl.field[i]));
        put(e_y, pl.ey, pl.ord_type);
        ENSURE(ctx->b_hstate, (size_t)pl.state_cells * sizeof(uint64_t));
        ENSURE(ctx->b_hedges, e_bytes);
        HIPCHK(hipMemsetAsync(ctx->b_hstate.p, 0, (size_t)pl.state_cells * sizeof(uint64_t), st));
        HIPCHK(hipMemcpyAsync(ctx->b_hedges.p, blob.data(), e_bytes, hipMemcpyHostToDevice, st));
        ctx->hpass.open = false;                  // (whatever fails from here on, no half-begun pass stays open)
    }
    const auto pow2_below = [](int n) { int s = 1; while (2 * s <= n) s *= 2; return n > 0 ? s : 0; };
    const long block_gates = pl.rows_per_block * (long)ng;
    const long stretches = cdiv(block_gates, (long)HIST_STRETCH);
    for (int i = 0; i < pl.n_fields; ++i) {
        const int k = pl.field[i];
        HistArgs ha{};
        ha.x = in[k]; ha.y = y;
        ha.ex = (const char *)ctx->b_hedges.p + e_off[k];
        ha.ey = (const char *)ctx->b_hedges.p + e_y;
        ha.state = (unsigned long long *)ctx->b_hstate.p + pl.state_off[k];
        ha.block_gates = block_gates;
        ha.y_gates = y_gates > 0 ? y_gates : n_rg;
        ha.n_ex = pl.n_ex[k]; ha.n_ey = pl.n_ey;
        ha.step_x = pow2_below(pl.n_ex[k]); ha.step_y = pow2_below(pl.n_ey);
        ha.nx2 = pl.n_ex[k] + 1;
        ha.cells = pl.cells[k];
        ha.stretches = (int)stretches;
        const bool x64 = hist_field_type(k) == HIST_T_F64;
        const size_t lds = (((size_t)pl.n_ex[k] * (x64 ? 8 : 4) + 7) & ~(size_t)7) +
                           (pl.ord_type == HIST_T_NONE ? 0 : (((size_t)pl.n_ey * (pl.ord_type == HIST_T_F64 ? 8 : 4) + 7) & ~(size_t)7)) +
                           (size_t)pl.cells[k] * sizeof(unsigned);
        const void *fn = nullptr;
        size_t &allowed = root_of(ctx)->hist_lds_allowed[x64 ? 1 : 0][pl.ord_type];
        if (lds > allowed) {
            // beyond the default 64 KB per workgroup: ask for it (an attribute of the kernel's instantiation; the largest
            // request so far is kept)
            hist_launch_field(x64, pl.ord_type, 0, 0, st, ha, &fn);
            HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            allowed = lds;
        }
        const unsigned grid = (unsigned)(pl.n_blocks * stretches);
        hist_launch_field(x64, pl.ord_type, grid, lds, st, ha, &fn);
        HIPCHK(hipGetLastError());
    }
    if (pl.finish)
        for (int i = 0; i < pl.n_fields; ++i) {
            const int k = pl.field[i];
            HIPCHK(hipMemcpyAsync(T[k], (const unsigned long long *)ctx->b_hstate.p + pl.state_off[k],
                                  (size_t)pl.n_blocks * pl.cells[k] * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        }
    try {
        hist_advance(h, pl, &ctx->hpass);
    } catch (...) {
        ctx->hpass.open = false;
        ctx->err = "cpol_histogram: out of host memory";
        return CPOL_ERR_NOMEM;
    }
    return CPOL_OK;
}

// The test hook cpol_debug_read "histogram_fields": k_hist and the running state on caller-supplied rows (host memory in, host
// memory out, blocking) -- the kernel on rows no sweep produces (every value class, every stretch length, the largest tables).
struct HistHook {
    int32_t n_rows, n_gates, n_rays, n_model_vars;
    const void *in[CPOL_HIST_FIELDS];       // [n_rows * n_gates] float32 (slot RVEL float64); NULL = not given
    const float *heights, *dist;            // [n_rays * n_gates]
    const double *model_vars;               // [n_model_vars][n_rows * n_gates]
    cpol_histogram h;
};

static int hist_hook(cpol_ctx *ctx, const HistHook *hk)
{
    if (hk->n_rows < 1 || hk->n_gates < 1 || (long)hk->n_rows * hk->n_gates >= (1L << 31) || hk->n_rays < 1 || hk->n_rows % hk->n_rays != 0 ||
        hk->n_model_vars < 0 || hk->n_model_vars > CPOL_MAX_VARS) {
        ctx->err = "histogram_fields: bad shape (n_rays divides n_rows)";
        return CPOL_ERR_ARG;
    }
    HistCall c;
    c.n_rows = hk->n_rows; c.n_gates = hk->n_gates; c.doppler = true; c.n_model_vars = hk->model_vars ? hk->n_model_vars : 0;
    HistPlan pl;
    PlaceArray arr[CPOL_HIST_FIELDS];
    int rc = hist_plan(ctx, &hk->h, c, &pl, arr);
    if (rc != CPOL_OK) return rc;
    const int ord = hk->h.ordinate;
    const int ord_field = (ord >= HIST_ORD_FIELD && ord < HIST_ORD_FIELD + CPOL_HIST_FIELDS) ? ord - HIST_ORD_FIELD : -1;
    for (int k = 0; k < CPOL_HIST_FIELDS; ++k)
        if ((pl.cells[k] || k == ord_field) && !hk->in[k]) { ctx->err = "histogram_fields: a requested field or the ordinate has no input"; return CPOL_ERR_ARG; }
    if ((ord == HIST_ORD_HEIGHTS && !hk->heights) || (ord == HIST_ORD_DIST && !hk->dist)) { ctx->err = "histogram_fields: the ordinate has no input"; return CPOL_ERR_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)hk->n_rows * hk->n_gates, n_geo = (size_t)hk->n_rays * hk->n_gates;
    const void *in[CPOL_HIST_FIELDS] = {};
    if ((rc = hook_upload_fields(ctx, hk->in, CPOL_HIST_FIELDS, ~0u, n, in)) != CPOL_OK) return rc;
    const void *y = nullptr;
    long y_gates = (long)n;
    if (ord == HIST_ORD_HEIGHTS || ord == HIST_ORD_DIST) {
        DevBuf &b = ctx->b_out[ord == HIST_ORD_HEIGHTS ? 13 : 12];
        if ((rc = upload(ctx, b, ord == HIST_ORD_HEIGHTS ? hk->heights : hk->dist, n_geo * sizeof(float))) != CPOL_OK) return rc;
        y = b.p; y_gates = (long)n_geo;
    } else if (ord_field >= 0) y = in[ord_field];
    else if (ord >= HIST_ORD_MODEL) {
        if ((rc = upload(ctx, ctx->b_model, hk->model_vars, (size_t)hk->n_model_vars * n * sizeof(double))) != CPOL_OK) return rc;
        y = (const double *)ctx->b_model.p + (size_t)(ord - HIST_ORD_MODEL) * n;
    }
    DevBuf *own[CPOL_HIST_FIELDS];
    for (int k = 0; k < CPOL_HIST_FIELDS; ++k) own[k] = &ctx->b_hcounts[k];
    return hook_finish(ctx, arr, own, [&](void *const *T) { return hist_launch(ctx, &hk->h, pl, in, y, y_gates, (long)n, hk->n_gates, T, ctx->stream); });
}

// ---- hydrometeor contributions (cpol_species, k_species in cpol_species.inl): the checks and the launch, shared by the launch
// sequence and the test hook ----
// every refusal of a cpol_species for a call of n_rg gates and n_hyd staged slots; queues nothing.  arr[SP_N]: the caller's arrays
// for the placement plan (cpol_place.h): arrays of the sweep itself, each with a grow-only buffer of its own, made only when asked for
static int species_plan(cpol_ctx *ctx, const cpol_species *sp, long n_rg, int n_hyd, PlaceArray *arr)
{
    auto bad = [&](const char *why) { ctx->err = std::string("cpol_species: ") + why; return CPOL_ERR_ARG; };
    void *const f[SP_N] = {sp->ZH, sp->ZV, sp->ZDR, sp->KDP, sp->RHOHV, sp->DELTA_HV, sp->ATT_H, sp->ATT_V, sp->dominant, sp->present,
                           sp->share, sp->sz};
    bool any = false;
    for (int k = 0; k < SP_N; ++k) any = any || f[k] != nullptr;
    if (!any) return bad("every output pointer is NULL");
    if (sp->n_hydro != n_hyd) return bad("n_hydro must equal the staged hydrometeor slots");
    for (int k = 0; k < SP_N; ++k) {
        arr[k] = PlaceArray{};
        arr[k].user = (uintptr_t)f[k];
        arr[k].bytes = k < SP_FIELDS ? (size_t)n_hyd * n_rg * sizeof(float) : k == SP_SHARE ? (size_t)n_rg * sizeof(float)
                     : k == SP_SZ ? (size_t)n_rg * n_hyd * CPOL_N_SZ * sizeof(float) : (size_t)n_rg;
        arr[k].produced = f[k] != nullptr;
        arr[k].product = PLACE_SWEEP;
    }
    return CPOL_OK;
}

// sz_integ [n_rg][n_hyd][12] and zh_final [n_rg]: device arrays; T: where the kernel writes (NULL: not asked for).  ONE kernel;
// the rows themselves, when asked for, are a device-to-device copy
static int species_launch(cpol_ctx *ctx, const float *sz_integ, const float *zh_final, void *const T[SP_N], long n_rg, int n_hyd,
                          float c_zh, float c_kdp, float c_2w, hipStream_t st)
{
    SpeciesArgs sa{};
    sa.sz_integ = sz_integ; sa.zh_final = zh_final;
    bool any = false;
    for (int k = 0; k < SP_FIELDS; ++k) { sa.f[k] = (float *)T[k]; any = any || T[k]; }
    sa.dominant = (unsigned char *)T[SP_DOMINANT]; sa.present = (unsigned char *)T[SP_PRESENT]; sa.share = (float *)T[SP_SHARE];
    any = any || sa.dominant || sa.present || sa.share;
    sa.n_rg = n_rg; sa.n_hydro = n_hyd;
    sa.c_zh = c_zh; sa.c_kdp = c_kdp; sa.c_2w = c_2w;
    if (any) {
        hipLaunchKernelGGL(k_species, dim3((unsigned)cdiv(n_rg, (long)CPOL_SPECIES_THREADS)), dim3(CPOL_SPECIES_THREADS), 0, st, sa);
        HIPCHK(hipGetLastError());
    }
    if (T[SP_SZ]) HIPCHK(hipMemcpyAsync(T[SP_SZ], sz_integ, (size_t)n_rg * n_hyd * CPOL_N_SZ * sizeof(float), hipMemcpyDeviceToDevice, st));
    return CPOL_OK;
}

// The test hook cpol_debug_read "species_fields": k_species alone on caller-supplied rows (host memory in, host memory out,
// blocking) -- the kernel on rows no sweep produces (zeros of either sign, infinities, ties, empty and censored gates).
struct SpeciesHook {
    int32_t n_rows, n_gates;
    const float *sz;                        // [n_rows * n_gates][sp.n_hydro][12]
    const float *zh_final;                  // [n_rows * n_gates]
    float c_zh, c_kdp, c_2w, pad_;
    cpol_species sp;                        // host output pointers
};

static int species_hook(cpol_ctx *ctx, const SpeciesHook *hk)
{
    if (hk->n_rows < 1 || hk->n_gates < 1 || (long)hk->n_rows * hk->n_gates >= (1L << 31) || hk->sp.n_hydro < 1 ||
        hk->sp.n_hydro > CPOL_MAX_HYDRO || !hk->sz || !hk->zh_final) {
        ctx->err = "species_fields: bad shape (n_rows, n_gates >= 1, n_hydro in 1 ... CPOL_MAX_HYDRO) or a NULL input";
        return CPOL_ERR_ARG;
    }
    const long n = (long)hk->n_rows * hk->n_gates;
    const int n_hyd = hk->sp.n_hydro;
    PlaceArray arr[SP_N];
    int rc = species_plan(ctx, &hk->sp, n, n_hyd, arr);
    if (rc != CPOL_OK) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = upload(ctx, ctx->b_szinteg, hk->sz, (size_t)n * n_hyd * CPOL_N_SZ * sizeof(float))) != CPOL_OK) return rc;
    if ((rc = upload(ctx, ctx->b_out[0], hk->zh_final, (size_t)n * sizeof(float))) != CPOL_OK) return rc;
    DevBuf *own[SP_N];
    for (int k = 0; k < SP_N; ++k) own[k] = &ctx->b_spout[k];
    return hook_finish(ctx, arr, own, [&](void *const *T) {
        return species_launch(ctx, (const float *)ctx->b_szinteg.p, (const float *)ctx->b_out[0].p, T, n, n_hyd, hk->c_zh, hk->c_kdp, hk->c_2w,
                              ctx->stream);
    });
}

// ---- gridded composites (cpol_composite, k_comp and k_comp_finish in cpol_comp.inl): the checks (cpol_comp.h), the pass and the
// launches, shared by the launch sequence and the test hook ----
#ifndef CPOL_COMP_COMBINE
#define CPOL_COMP_COMBINE 1        // the kept lane form of k_comp: 1 lanes that share a cell combined inside the wavefront, 0 every lane on its own
#endif
enum { CP_COUNT = CPOL_COMP_FIELDS, CP_COLUMN, CP_LAYERS = CP_COLUMN + CPOL_COMP_FIELDS, CP_SUM = CP_LAYERS + CPOL_COMP_FIELDS,
       CP_SKIPPED = CP_SUM + CPOL_COMP_FIELDS, CP_N = CP_SKIPPED + CPOL_COMP_FIELDS };
static_assert(CP_N == 5 * CPOL_COMP_FIELDS + 1, "cpol_ctx::b_cout holds one buffer per array");
#ifndef CPOL_COMP_SUM_COMBINE
#define CPOL_COMP_SUM_COMBINE 1    // the kept lane form of k_comp_sum: 1 the runs of equal (cell, bin) summed inside the wavefront, 0 every lane on its own
#endif
// every refusal of a cpol_composite for the call `c`; queues nothing and leaves the pass as it is.  arr[CP_N]: the caller's nine
// `values`, `count`, with height layers the nine `column` and `column_layers`, and with the exact sums the nine `sum` and
// `sum_skipped`, for the placement plan (cpol_place.h): arrays
// of the sweep itself, each with a grow-only buffer of its own, produced by a finishing call alone
static int comp_plan(cpol_ctx *ctx, const cpol_composite *c, const CompCall &call, CompPlan *pl, PlaceArray *arr)
{
    const char *why = nullptr;
    try {
        why = comp_check(c, call, ctx->cpass, pl);
    } catch (...) {
        ctx->err = "cpol_composite: out of host memory";
        return CPOL_ERR_NOMEM;
    }
    if (why) { ctx->err = std::string("cpol_composite: ") + why; return CPOL_ERR_ARG; }
    for (int k = 0; k < CP_N; ++k) arr[k] = PlaceArray{};
    if (!pl->finish) return CPOL_OK;
    for (int i = 0; i < pl->n_fields; ++i) {
        const int k = pl->field[i];
        arr[k].user = (uintptr_t)c->values[k];
        arr[k].bytes = (size_t)pl->n_blocks * pl->n_planes[k] * pl->block_cells * sizeof(float);
        arr[k].produced = true;
        arr[k].product = PLACE_SWEEP;
        if (pl->sum) {
            const cpol_composite_sums *const cs = (const cpol_composite_sums *)c;     // (the bit is set: comp_check)
            arr[CP_SUM + k].user = (uintptr_t)cs->sum[k];
            arr[CP_SUM + k].bytes = (size_t)pl->n_blocks * pl->block_cells * sizeof(double);
            arr[CP_SKIPPED + k].user = (uintptr_t)cs->sum_skipped[k];
            arr[CP_SKIPPED + k].bytes = (size_t)pl->n_blocks * pl->block_cells * sizeof(uint32_t);
            arr[CP_SUM + k].produced = arr[CP_SKIPPED + k].produced = true;
            arr[CP_SUM + k].product = arr[CP_SKIPPED + k].product = PLACE_SWEEP;
        }
        if (pl->tv[k].empty()) continue;
        arr[CP_COLUMN + k].user = (uintptr_t)c->column[k];
        arr[CP_COLUMN + k].bytes = (size_t)pl->n_blocks * pl->cells * sizeof(double);
        arr[CP_LAYERS + k].user = (uintptr_t)c->column_layers[k];
        arr[CP_LAYERS + k].bytes = (size_t)pl->n_blocks * pl->cells;
        arr[CP_COLUMN + k].produced = arr[CP_LAYERS + k].produced = true;
        arr[CP_COLUMN + k].product = arr[CP_LAYERS + k].product = PLACE_SWEEP;
    }
    arr[CP_COUNT].user = (uintptr_t)c->count;
    arr[CP_COUNT].bytes = (size_t)pl->n_blocks * pl->n_fields * pl->block_cells * sizeof(uint64_t);
    arr[CP_COUNT].produced = true;
    arr[CP_COUNT].product = PLACE_SWEEP;
    return CPOL_OK;
}

// in: the per-gate device arrays in the order of the fields; dist, hgt: the geometry's device arrays, holding geo_rays rows of ng
// gates; n_rg: the gates of the call; T: where a finishing call's maps go (nine `values`, then `count`); lane_form: 0 the kept
// form of k_comp, 1 combined, 2 every lane on its own; plane_on_host: gate_x / gate_y of a gate plane are host arrays (copied on
// `st`, or found in the plane store under plane_version), else memory the device reads in place.  Begins, composes (a SOURCE
// pass: into the scratch state, then k_comp_merge), finishes; then the pass is advanced
static int comp_launch(cpol_ctx *ctx, const cpol_composite *c, const CompPlan &pl, const void *const in[CPOL_COMP_FIELDS], const void *dist,
                       const void *hgt, int geo_rays, long n_rg, int ng, void *const T[CP_N], int lane_form, bool plane_on_host, hipStream_t st)
{
    const size_t n_ex = (size_t)pl.n_x + 1, n_ey = (size_t)pl.n_y + 1;
    if (pl.begin) {
        std::vector<double> &blob = ctx->cedges_host;     // (kept by the context: it outlives the copy whatever the runtime does)
        try {
            blob.assign(pl.ex.begin(), pl.ex.end());
            blob.insert(blob.end(), pl.ey.begin(), pl.ey.end());
        } catch (...) { ctx->err = "cpol_composite: out of host memory"; return CPOL_ERR_NOMEM; }
        ENSURE(ctx->b_cstate, (size_t)pl.total_bytes);
        ENSURE(ctx->b_cedges, (n_ex + n_ey) * sizeof(double));
        // the begin values: max states and counts 0, min states all ones; SOURCE: the source bytes behind them all ones too
        // (255), then the scratch state like the running one
        HIPCHK(hipMemsetAsync(ctx->b_cstate.p, 0, (size_t)pl.zero_bytes, st));
        const long ones_end = pl.with_source ? pl.off_scratch : pl.state_bytes;
        if (ones_end > pl.zero_bytes)
            HIPCHK(hipMemsetAsync((char *)ctx->b_cstate.p + pl.zero_bytes, 0xFF, (size_t)(ones_end - pl.zero_bytes), st));
        if (pl.with_source) {
            char *const scratch = (char *)ctx->b_cstate.p + pl.off_scratch;
            HIPCHK(hipMemsetAsync(scratch, 0, (size_t)pl.zero_bytes, st));
            if (pl.state_bytes > pl.zero_bytes)
                HIPCHK(hipMemsetAsync(scratch + pl.zero_bytes, 0xFF, (size_t)(pl.state_bytes - pl.zero_bytes), st));
        }
        HIPCHK(hipMemcpyAsync(ctx->b_cedges.p, blob.data(), (n_ex + n_ey) * sizeof(double), hipMemcpyHostToDevice, st));
        ctx->cpass.open = false;                  // (whatever fails from here on, no half-begun pass stays open)
        if (pl.n_z) {
            // the layer edges and the tables: COMP_TAB_EDGE_WORDS doubles' room for the 65 float32 edges, then per field with a
            // table n doubles and n floats (rounded up to whole doubles), in the order of the fields
            std::vector<double> &tab = ctx->ctab_host;
            try {
                size_t words = COMP_TAB_EDGE_WORDS;
                for (int k = 0; k < CPOL_COMP_FIELDS; ++k) words += pl.tv[k].size() + (pl.tv[k].size() + 1) / 2;
                tab.assign(words, 0.0);
            } catch (...) { ctx->err = "cpol_composite: out of host memory"; return CPOL_ERR_NOMEM; }
            memcpy(tab.data(), pl.ez.data(), pl.ez.size() * sizeof(float));
            size_t at_word = COMP_TAB_EDGE_WORDS;
            for (int k = 0; k < CPOL_COMP_FIELDS; ++k) {
                const size_t n = pl.tv[k].size();
                if (!n) continue;
                memcpy(tab.data() + at_word, pl.tf[k].data(), n * sizeof(double));
                memcpy(tab.data() + at_word + n, pl.tv[k].data(), n * sizeof(float));
                at_word += n + (n + 1) / 2;
            }
            ENSURE(ctx->b_ctab, tab.size() * sizeof(double));
            HIPCHK(hipMemcpyAsync(ctx->b_ctab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st));
        }
        if (pl.sum) {
            // the weight tables: per field with one n doubles and n floats (rounded up to whole doubles), in the order of the fields
            std::vector<double> &tab = ctx->cwtab_host;
            try {
                size_t words = 0;
                for (int k = 0; k < CPOL_COMP_FIELDS; ++k) words += pl.wv[k].size() + (pl.wv[k].size() + 1) / 2;
                tab.assign(words, 0.0);
            } catch (...) { ctx->err = "cpol_composite: out of host memory"; return CPOL_ERR_NOMEM; }
            size_t at_word = 0;
            for (int k = 0; k < CPOL_COMP_FIELDS; ++k) {
                const size_t n = pl.wv[k].size();
                if (!n) continue;
                memcpy(tab.data() + at_word, pl.wf[k].data(), n * sizeof(double));
                memcpy(tab.data() + at_word + n, pl.wv[k].data(), n * sizeof(float));
                at_word += n + (n + 1) / 2;
            }
            if (!tab.empty()) {
                ENSURE(ctx->b_cwtab, tab.size() * sizeof(double));
                HIPCHK(hipMemcpyAsync(ctx->b_cwtab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st));
            }
        }
    }
    const bool gates = pl.plane == CPOL_COMP_PLANE_GATES;
    const double *gx = nullptr, *gy = nullptr;
    if (!gates) {
        // the per-ray sines and cosines of this call
        ENSURE(ctx->b_crays, 2 * (size_t)geo_rays * sizeof(double));
        HIPCHK(hipMemcpyAsync(ctx->b_crays.p, c->ray_sin, (size_t)geo_rays * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((double *)ctx->b_crays.p + geo_rays, c->ray_cos, (size_t)geo_rays * sizeof(double), hipMemcpyHostToDevice, st));
    } else if (!plane_on_host) {
        gx = c->gate_x; gy = c->gate_y;
    } else {
        // the caller's per-gate coordinates: under a tag the store's copy (an upload on a miss, into the entry used longest ago),
        // without one a copy per call
        const size_t n_geo = (size_t)geo_rays * (size_t)ng;
        DevBuf *buf = &ctx->b_cplane;
        bool copy = true;
        if (c->plane_version) {
            cpol_ctx::CompPlane *e = nullptr, *lru = &ctx->cplanes[0];
            for (auto &q : ctx->cplanes) {
                if (q.version == c->plane_version && q.gates == n_geo && q.buf.p) { e = &q; break; }
                if (q.last_use < lru->last_use) lru = &q;
            }
            copy = e == nullptr;
            if (!e) { e = lru; e->version = 0; }
            e->last_use = ++ctx->cplane_clock;
            buf = &e->buf;
            if (copy) {
                ENSURE(*buf, 2 * n_geo * sizeof(double));
                e->gates = n_geo;
            }
            ctx->cplane_stat[copy ? 0 : 1] += 1;
            if (copy) {
                HIPCHK(hipMemcpyAsync(buf->p, c->gate_x, n_geo * sizeof(double), hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync((double *)buf->p + n_geo, c->gate_y, n_geo * sizeof(double), hipMemcpyHostToDevice, st));
                e->version = c->plane_version;
            }
        } else {
            ENSURE(*buf, 2 * n_geo * sizeof(double));
            HIPCHK(hipMemcpyAsync(buf->p, c->gate_x, n_geo * sizeof(double), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync((double *)buf->p + n_geo, c->gate_y, n_geo * sizeof(double), hipMemcpyHostToDevice, st));
        }
        gx = (const double *)buf->p; gy = gx + n_geo;
    }
    const auto pow2_below = [](int n) { int s = 1; while (2 * s <= n) s *= 2; return n > 0 ? s : 0; };
    const long block_gates = pl.rows_per_block * (long)ng;
    const long stretches = cdiv(block_gates, (long)COMP_STRETCH);
    char *const base = (char *)ctx->b_cstate.p;
    const auto at = [&](long off) { return off < 0 ? nullptr : base + off; };
    // (a SOURCE pass: k_comp fills the per-call scratch state, which has the offsets of the running one)
    const long into = pl.with_source ? pl.off_scratch : 0;
    const auto st_at = [&](long off) { return off < 0 ? nullptr : base + into + off; };
    const bool combine = lane_form == 0 ? CPOL_COMP_COMBINE != 0 : lane_form == 1;
    const bool sum_combine = lane_form == 0 ? CPOL_COMP_SUM_COMBINE != 0 : lane_form == 1;
    size_t w_word = 0;              // where the field's weight table begins in b_cwtab
    for (int i = 0; i < pl.n_fields; ++i) {
        const int k = pl.field[i];
        CompArgs ca{};
        ca.v = (const float *)in[k]; ca.dist = (const float *)dist; ca.hgt = (const float *)hgt;
        ca.ex = (const double *)ctx->b_cedges.p; ca.ey = ca.ex + n_ex;
        ca.ray_sin = (const double *)ctx->b_crays.p; ca.ray_cos = ca.ray_sin + geo_rays;
        ca.gx = gx; ca.gy = gy;
        ca.smax = (unsigned long long *)st_at(pl.off_max[k]); ca.slow = (unsigned long long *)st_at(pl.off_low[k]);
        ca.scount = (unsigned long long *)st_at(pl.off_count[k]); ca.stop = (unsigned *)st_at(pl.off_top[k]);
        ca.block_gates = block_gates;
        ca.geo_gates = (long)geo_rays * ng;
        ca.n_gates = ng;
        ca.n_ex = (int)n_ex; ca.n_ey = (int)n_ey;
        ca.step_x = pow2_below((int)n_ex); ca.step_y = pow2_below((int)n_ey);
        ca.n_x = pl.n_x; ca.n_y = pl.n_y; ca.cells = (int)pl.cells;
        ca.ez = (const float *)ctx->b_ctab.p; ca.n_z = pl.n_z; ca.step_z = pow2_below(pl.n_z + 1); ca.block_cells = pl.block_cells;
        ca.stretches = (int)stretches;
        ca.n_thr = pl.n_thr[k]; ca.slab = pl.slab ? 1 : 0;
        ca.h_lo = pl.h_lo; ca.h_hi = pl.h_hi;
        for (int j = 0; j < pl.n_thr[k]; ++j) ca.thr[j] = pl.thr[k][(size_t)j];
        const unsigned grid = (unsigned)(pl.n_blocks * stretches);
        const size_t lds = (n_ex + n_ey) * sizeof(double) + (pl.n_z ? (size_t)(pl.n_z + 1) * sizeof(float) : 0);          // (at most 16 KiB + 260 B)
        if (pl.n_z) {
            if (gates) {
                if (combine) hipLaunchKernelGGL((k_comp<true, true, true>), dim3(grid), dim3(COMP_THREADS), lds, st, ca);
                else hipLaunchKernelGGL((k_comp<false, true, true>), dim3(grid), dim3(COMP_THREADS), lds, st, ca);
            } else {
                if (combine) hipLaunchKernelGGL((k_comp<true, false, true>), dim3(grid), dim3(COMP_THREADS), lds, st, ca);
                else hipLaunchKernelGGL((k_comp<false, false, true>), dim3(grid), dim3(COMP_THREADS), lds, st, ca);
            }
        } else if (gates) {
            if (combine) hipLaunchKernelGGL((k_comp<true, true>), dim3(grid), dim3(COMP_THREADS), lds, st, ca);
            else hipLaunchKernelGGL((k_comp<false, true>), dim3(grid), dim3(COMP_THREADS), lds, st, ca);
        } else {
            if (combine) hipLaunchKernelGGL((k_comp<true, false>), dim3(grid), dim3(COMP_THREADS), lds, st, ca);
            else hipLaunchKernelGGL((k_comp<false, false>), dim3(grid), dim3(COMP_THREADS), lds, st, ca);
        }
        HIPCHK(hipGetLastError());
        if (pl.with_source) {
            CompMergeArgs ma{};
            ma.rmax = (unsigned long long *)at(pl.off_max[k]); ma.rlow = (unsigned long long *)at(pl.off_low[k]);
            ma.rcount = (unsigned long long *)at(pl.off_count[k]); ma.rtop = (unsigned *)at(pl.off_top[k]);
            ma.smax = ca.smax; ma.slow = ca.slow; ma.scount = ca.scount; ma.stop = ca.stop;
            ma.bmax = (unsigned char *)at(pl.off_src_max[k]); ma.blow = (unsigned char *)at(pl.off_src_low[k]);
            ma.n = pl.n_blocks * pl.cells;
            ma.cells = (int)pl.cells; ma.n_thr = pl.n_thr[k];
            ma.source = (unsigned)pl.source;
            hipLaunchKernelGGL(k_comp_merge, dim3((unsigned)cdiv(ma.n, (long)COMP_THREADS)), dim3(COMP_THREADS), 0, st, ma);
            HIPCHK(hipGetLastError());
        }
        if (pl.sum) {
            // the exact sums of this field, behind its k_comp: the same grid, the same stretches (comp_check refuses SUM with SOURCE)
            CompSumArgs sa{};
            sa.a = ca;
            sa.a.smax = sa.a.slow = sa.a.scount = nullptr; sa.a.stop = nullptr;
            const size_t nw = pl.wv[k].size();
            sa.n_w = (int)nw; sa.step_w = pow2_below((int)nw);
            if (nw) {
                sa.wf = (const double *)ctx->b_cwtab.p + w_word; sa.wv = (const float *)(sa.wf + nw);
                w_word += nw + (nw + 1) / 2;
            }
            sa.bins = (unsigned long long *)at(pl.off_sum[k]); sa.skipped = (unsigned *)at(pl.off_skip[k]);
            const size_t slds = (n_ex + n_ey + nw) * sizeof(double) + (nw + (pl.n_z ? (size_t)pl.n_z + 1 : 0)) * sizeof(float);   // (at most 28 KiB + 260 B)
            if (pl.n_z) {
                if (gates) {
                    if (sum_combine) hipLaunchKernelGGL((k_comp_sum<true, true, true>), dim3(grid), dim3(COMP_THREADS), slds, st, sa);
                    else hipLaunchKernelGGL((k_comp_sum<false, true, true>), dim3(grid), dim3(COMP_THREADS), slds, st, sa);
                } else {
                    if (sum_combine) hipLaunchKernelGGL((k_comp_sum<true, false, true>), dim3(grid), dim3(COMP_THREADS), slds, st, sa);
                    else hipLaunchKernelGGL((k_comp_sum<false, false, true>), dim3(grid), dim3(COMP_THREADS), slds, st, sa);
                }
            } else if (gates) {
                if (sum_combine) hipLaunchKernelGGL((k_comp_sum<true, true, false>), dim3(grid), dim3(COMP_THREADS), slds, st, sa);
                else hipLaunchKernelGGL((k_comp_sum<false, true, false>), dim3(grid), dim3(COMP_THREADS), slds, st, sa);
            } else {
                if (sum_combine) hipLaunchKernelGGL((k_comp_sum<true, false, false>), dim3(grid), dim3(COMP_THREADS), slds, st, sa);
                else hipLaunchKernelGGL((k_comp_sum<false, false, false>), dim3(grid), dim3(COMP_THREADS), slds, st, sa);
            }
            HIPCHK(hipGetLastError());
        }
    }
    if (pl.finish)
        for (int i = 0; i < pl.n_fields; ++i) {
            const int k = pl.field[i];
            CompFinishArgs fa{};
            fa.smax = (const unsigned long long *)at(pl.off_max[k]); fa.slow = (const unsigned long long *)at(pl.off_low[k]);
            fa.scount = (const unsigned long long *)at(pl.off_count[k]); fa.stop = (const unsigned *)at(pl.off_top[k]);
            fa.values = (float *)T[k];
            fa.count = (unsigned long long *)T[CP_COUNT] + (size_t)pl.slot[k] * pl.cells;
            fa.n = pl.n_blocks * pl.block_cells;            // (height layers: n_blocks * n_z blocks of `cells`)
            fa.cells = (int)pl.cells; fa.n_planes = pl.n_planes[k]; fa.n_fields = pl.n_fields; fa.n_thr = pl.n_thr[k];
            fa.bmax = (const unsigned char *)at(pl.off_src_max[k]); fa.blow = (const unsigned char *)at(pl.off_src_low[k]);
            hipLaunchKernelGGL(k_comp_finish, dim3((unsigned)cdiv(fa.n, (long)COMP_THREADS)), dim3(COMP_THREADS), 0, st, fa);
            HIPCHK(hipGetLastError());
            if (!pl.sum) continue;
            CompSumFinishArgs sf{};
            sf.bins = (const unsigned long long *)at(pl.off_sum[k]); sf.skipped = (const unsigned *)at(pl.off_skip[k]);
            sf.scount = fa.scount;
            sf.sum = (double *)T[CP_SUM + k]; sf.sum_skipped = (unsigned *)T[CP_SKIPPED + k];
            sf.n = fa.n;
            hipLaunchKernelGGL(k_comp_sum_finish, dim3((unsigned)cdiv(sf.n, (long)COMP_THREADS)), dim3(COMP_THREADS), 0, st, sf);
            HIPCHK(hipGetLastError());
        }
    if (pl.finish && pl.column) {
        // the column integrals: one launch per field with a table, behind k_comp_finish (it reads the MAX states alone)
        size_t at_word = COMP_TAB_EDGE_WORDS;
        for (int k = 0; k < CPOL_COMP_FIELDS; ++k) {
            const size_t n = pl.tv[k].size();
            if (!n) continue;
            CompColumnArgs co{};
            co.smax = (const unsigned long long *)at(pl.off_max[k]);
            co.tf = (const double *)ctx->b_ctab.p + at_word;
            co.tv = (const float *)(co.tf + n);
            co.ez = (const float *)ctx->b_ctab.p;
            co.column = (double *)T[CP_COLUMN + k];
            co.layers = (unsigned char *)T[CP_LAYERS + k];
            co.n = pl.n_blocks * pl.cells;
            co.cells = (int)pl.cells; co.n_z = pl.n_z; co.n_tab = (int)n; co.step_t = pow2_below((int)n); co.gaps = pl.gaps;
            hipLaunchKernelGGL(k_comp_column, dim3((unsigned)cdiv(co.n, (long)COMP_THREADS)), dim3(COMP_THREADS), 0, st, co);
            HIPCHK(hipGetLastError());
            at_word += n + (n + 1) / 2;
        }
    }
    (void)n_rg;
    try {
        comp_advance(c, pl, &ctx->cpass);
    } catch (...) {
        ctx->cpass.open = false;
        ctx->err = "cpol_composite: out of host memory";
        return CPOL_ERR_NOMEM;
    }
    return CPOL_OK;
}

// The test hook cpol_debug_read "composite_fields": the plan, the placement, both kernels and the running state on
// caller-supplied rows (host memory in, host memory out, blocking) -- the kernels on rows no sweep produces (every value class,
// every stretch length, runs of equal cells across wavefront and workgroup boundaries, the largest grids).
struct CompHook {
    int32_t n_rows, n_gates, n_rays, lane_form;
    const float *in[CPOL_COMP_FIELDS];      // [n_rows * n_gates]; NULL = not given
    const float *heights, *dist;            // [n_rays * n_gates]; dist may be NULL on a gate plane (c.gate_x, c.gate_y: host arrays)
    cpol_composite c;               // with CPOL_COMP_SUM in c.products: the member `c` of a cpol_composite_sums, the last member of the hook's struct
};

static int comp_hook(cpol_ctx *ctx, const CompHook *hk)
{
    if (hk->n_rows < 1 || hk->n_gates < 1 || (long)hk->n_rows * hk->n_gates >= (1L << 31) || hk->n_rays < 1 || hk->n_rows % hk->n_rays != 0 ||
        hk->lane_form < 0 || hk->lane_form > 2) {
        ctx->err = "composite_fields: bad shape (n_rays divides n_rows) or lane form";
        return CPOL_ERR_ARG;
    }
    CompCall call;
    call.n_rows = hk->n_rows; call.n_gates = hk->n_gates;
    CompPlan pl;
    PlaceArray arr[CP_N];
    int rc = comp_plan(ctx, &hk->c, call, &pl, arr);
    if (rc != CPOL_OK) return rc;
    for (int i = 0; i < pl.n_fields; ++i)
        if (!hk->in[pl.field[i]]) { ctx->err = "composite_fields: a requested field has no input"; return CPOL_ERR_ARG; }
    const bool hk_gates = hk->c.plane == CPOL_COMP_PLANE_GATES;
    if (!hk->heights || (!hk->dist && !hk_gates)) { ctx->err = "composite_fields: heights and dist are needed"; return CPOL_ERR_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)hk->n_rows * hk->n_gates, n_geo = (size_t)hk->n_rays * hk->n_gates;
    const void *in[CPOL_COMP_FIELDS] = {};
    if ((rc = hook_upload_fields(ctx, (const void *const *)hk->in, CPOL_COMP_FIELDS, ~0u, n, in)) != CPOL_OK) return rc;
    if (hk->dist && (rc = upload(ctx, ctx->b_out[12], hk->dist, n_geo * sizeof(float))) != CPOL_OK) return rc;
    if ((rc = upload(ctx, ctx->b_out[13], hk->heights, n_geo * sizeof(float))) != CPOL_OK) return rc;
    DevBuf *own[CP_N];
    for (int k = 0; k < CP_N; ++k) own[k] = &ctx->b_cout[k];
    return hook_finish(ctx, arr, own, [&](void *const *T) {
        return comp_launch(ctx, &hk->c, pl, in, hk->dist ? ctx->b_out[12].p : nullptr, ctx->b_out[13].p, hk->n_rays, (long)n, hk->n_gates, T,
                           hk->lane_form, true, ctx->stream);
    });
}

// ---- neighbourhood verification (cpol_fractions, k_frac_rows / k_frac_cols / k_frac_score in cpol_frac.inl): the checks
// (cpol_frac.h) and the launches, shared by the launch sequence and the test hook ----
enum { FR_SUMS, FR_TOTALS, FR_OBJ_N, FR_OBJ_TABLE, FR_OBJ_LABELS, FR_OBJ_VOLUME, FR_OBJ_SKIPPED, FR_OBJ_FIELD, FR_OBJ_FIELD_CELLS,
       FR_OBJ_N_PIECES, FR_OBJ_PIECES, FR_OBJ_COVERED, FR_PROB_SUMS, FR_RELIABILITY, FR_MEMBER_SUM, FR_MEMBER_ANY,
       FR_TRACK_CORR, FR_TRACK_SHIFT, FR_TRACK_N, FR_TRACK_PIECES, FR_TRACK_COVERED, FR_N };
static_assert(FR_N == 21, "cpol_ctx::b_fout holds one buffer per array");
// arr[FR_N]: the caller's `sums` and `totals` for the placement plan (cpol_place.h): arrays of the sweep itself, like the
// composite's `count`; behind them n_objects, table and labels of the object cells (op.on; labels when asked for); last the four
// arrays of the neighbourhood ensemble probabilities (pl.prob.on; the two maps when asked for)
static void frac_place(const cpol_fractions *f, const FracPlan &pl, const ObjPlan &op, PlaceArray *arr)
{
    for (int k = 0; k < FR_N; ++k) { arr[k] = PlaceArray{}; arr[k].product = PLACE_SWEEP; }
    if (pl.prob.on) {
        const cpol_fraction_probabilities *const q = frac_probabilities(f);
        const FracProbPlan &pp = pl.prob;
        arr[FR_PROB_SUMS].user = (uintptr_t)q->prob_sums;      arr[FR_PROB_SUMS].bytes = pp.prob_sums_bytes;     arr[FR_PROB_SUMS].produced = true;
        arr[FR_RELIABILITY].user = (uintptr_t)q->reliability;  arr[FR_RELIABILITY].bytes = pp.reliability_bytes; arr[FR_RELIABILITY].produced = true;
        arr[FR_MEMBER_SUM].user = (uintptr_t)q->member_sum;    arr[FR_MEMBER_SUM].bytes = pp.member_sum_bytes;   arr[FR_MEMBER_SUM].produced = pp.member_sum;
        arr[FR_MEMBER_ANY].user = (uintptr_t)q->member_any;    arr[FR_MEMBER_ANY].bytes = pp.member_any_bytes;   arr[FR_MEMBER_ANY].produced = pp.member_any;
    }
    arr[FR_SUMS].user = (uintptr_t)f->sums;     arr[FR_SUMS].bytes = pl.sums_bytes;
    arr[FR_TOTALS].user = (uintptr_t)f->totals; arr[FR_TOTALS].bytes = pl.totals_bytes;
    arr[FR_SUMS].produced = arr[FR_TOTALS].produced = true;
    if (!op.on) return;
    const cpol_objects *const o = f->objects;
    arr[FR_OBJ_N].user = (uintptr_t)o->n_objects;    arr[FR_OBJ_N].bytes = op.n_bytes;           arr[FR_OBJ_N].produced = true;
    arr[FR_OBJ_TABLE].user = (uintptr_t)o->table;    arr[FR_OBJ_TABLE].bytes = op.table_bytes;   arr[FR_OBJ_TABLE].produced = true;
    arr[FR_OBJ_LABELS].user = (uintptr_t)o->labels;  arr[FR_OBJ_LABELS].bytes = op.labels_bytes; arr[FR_OBJ_LABELS].produced = op.labels;
    if (op.match) {
        const cpol_objects_match *const mo = (const cpol_objects_match *)o;       // (o->pad_ != 0: obj_check)
        arr[FR_OBJ_N_PIECES].user = (uintptr_t)mo->n_pieces;  arr[FR_OBJ_N_PIECES].bytes = op.n_pieces_bytes;  arr[FR_OBJ_N_PIECES].produced = true;
        arr[FR_OBJ_PIECES].user = (uintptr_t)mo->pieces;      arr[FR_OBJ_PIECES].bytes = op.pieces_bytes;      arr[FR_OBJ_PIECES].produced = true;
        arr[FR_OBJ_COVERED].user = (uintptr_t)mo->covered;    arr[FR_OBJ_COVERED].bytes = op.covered_bytes;    arr[FR_OBJ_COVERED].produced = true;
    }
    if (op.track) {
        const cpol_objects_track *const tr = (const cpol_objects_track *)o;       // (CPOL_OBJ_TRACK in o->pad_: obj_check)
        arr[FR_TRACK_CORR].user = (uintptr_t)tr->correlation; arr[FR_TRACK_CORR].bytes = op.track_corr_bytes;      arr[FR_TRACK_CORR].produced = op.track_corr_wanted;
        arr[FR_TRACK_SHIFT].user = (uintptr_t)tr->shift;      arr[FR_TRACK_SHIFT].bytes = op.track_shift_bytes;    arr[FR_TRACK_SHIFT].produced = true;
        arr[FR_TRACK_N].user = (uintptr_t)tr->n_pieces;       arr[FR_TRACK_N].bytes = op.track_n_bytes;            arr[FR_TRACK_N].produced = true;
        arr[FR_TRACK_PIECES].user = (uintptr_t)tr->pieces;    arr[FR_TRACK_PIECES].bytes = op.track_pieces_bytes;  arr[FR_TRACK_PIECES].produced = true;
        arr[FR_TRACK_COVERED].user = (uintptr_t)tr->covered;  arr[FR_TRACK_COVERED].bytes = op.track_covered_bytes; arr[FR_TRACK_COVERED].produced = true;
    }
    if (!op.sums) return;
    arr[FR_OBJ_VOLUME].user = (uintptr_t)o->volume;            arr[FR_OBJ_VOLUME].bytes = op.volume_bytes;           arr[FR_OBJ_VOLUME].produced = true;
    arr[FR_OBJ_SKIPPED].user = (uintptr_t)o->skipped;          arr[FR_OBJ_SKIPPED].bytes = op.skipped_bytes;         arr[FR_OBJ_SKIPPED].produced = true;
    arr[FR_OBJ_FIELD].user = (uintptr_t)o->field;              arr[FR_OBJ_FIELD].bytes = op.field_bytes;             arr[FR_OBJ_FIELD].produced = true;
    arr[FR_OBJ_FIELD_CELLS].user = (uintptr_t)o->field_cells;  arr[FR_OBJ_FIELD_CELLS].bytes = op.field_cells_bytes; arr[FR_OBJ_FIELD_CELLS].produced = true;
}

// the exact sums behind k_obj_decode; a: the arguments of the object kernels (its sums' members are filled here)
static int obj_launch_sums(cpol_ctx *ctx, ObjArgs a, const ObjPlan &op, void *const T[FR_N], hipStream_t st)
{
    const dim3 rows((unsigned)op.grid_rows), thr(OBJ_THREADS);
    // the exact sums: the accumulators behind the labelling scratch cleared, the weight table behind them
    char *const scr = (char *)ctx->b_oscr.p;
    a.acc = (unsigned long long *)(scr + op.acc_offset);
    a.volume = (double *)T[FR_OBJ_VOLUME]; a.skipped = (unsigned *)T[FR_OBJ_SKIPPED];
    a.field = (double *)T[FR_OBJ_FIELD]; a.field_cells = (unsigned *)T[FR_OBJ_FIELD_CELLS];
    const size_t nw = op.weight_v.size();
    a.n_weight = (int)nw;
    if (nw) {
        a.wf = (const double *)(scr + op.weight_offset); a.wv = (const float *)(a.wf + nw);
        for (a.step_w = 1; 2 * a.step_w <= (int)nw; a.step_w *= 2) {}
        HIPCHK(hipMemcpyAsync((void *)a.wf, op.weight_f.data(), nw * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((void *)a.wv, op.weight_v.data(), nw * sizeof(float), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemsetAsync(a.acc, 0, (size_t)op.acc_bytes, st));
    HIPCHK(hipMemsetAsync(a.skipped, 0, op.skipped_bytes, st));
    HIPCHK(hipMemsetAsync(a.field_cells, 0, op.field_cells_bytes, st));
    hipLaunchKernelGGL(k_obj_sums, rows, thr, 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_sums_finish, dim3((unsigned)op.grid_finish), thr, 0, st, a);
    HIPCHK(hipGetLastError());
    return CPOL_OK;
}

// the match behind everything else: the piece arrays of the scratch through the objects' own kernels (cpol_obj.inl); a: the
// arguments of the object kernels, whose L and aux k_obj_number left flattened and numbered
static int obj_launch_match(cpol_ctx *ctx, const ObjArgs &a, const ObjPlan &op, void *const T[FR_N], hipStream_t st)
{
    MatchArgs g{};
    g.L = a.L; g.aux = a.aux; g.max_objects = op.max_objects;
    g.covered = (unsigned *)T[FR_OBJ_COVERED];
    g.p.f = a.f;
    g.p.L = (unsigned *)((char *)ctx->b_oscr.p + op.piece_offset); g.p.aux = g.p.L + op.piece_maps * op.cells; g.p.rowcnt = g.p.aux + op.piece_maps * op.cells;
    g.p.n_objects = (unsigned *)T[FR_OBJ_N_PIECES]; g.p.table = (unsigned *)T[FR_OBJ_PIECES];
    g.p.n_maps = op.piece_maps;
    g.p.connectivity = op.connectivity; g.p.min_area = 1; g.p.max_objects = op.max_pieces;
    HIPCHK(hipMemsetAsync(T[FR_OBJ_PIECES], 0, op.pieces_bytes, st));
    HIPCHK(hipMemsetAsync(T[FR_OBJ_COVERED], 0, op.covered_bytes, st));
    const dim3 rows((unsigned)op.grid_piece_rows), thr(OBJ_THREADS);
    hipLaunchKernelGGL(k_match_runs, rows, thr, 0, st, g);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_merge, rows, thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_flatten, dim3((unsigned)op.grid_piece_cells), thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_area, rows, thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_count, rows, thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_number, rows, thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_match_attr, rows, thr, 0, st, g);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_match_decode, dim3((unsigned)op.grid_piece_decode), thr, 0, st, g);
    HIPCHK(hipGetLastError());
    return CPOL_OK;
}

// the track behind everything else: Ke of every block packed, the correlation and its argmax (or the given shifts copied into
// `shift`), then the track's own piece arrays through the objects' kernels as in obj_launch_match; a: as there
static int obj_launch_track(cpol_ctx *ctx, const ObjArgs &a, const ObjPlan &op, void *const T[FR_N], hipStream_t st)
{
    char *const scr = (char *)ctx->b_oscr.p;
    TrackArgs g{};
    g.L = a.L; g.aux = a.aux; g.max_objects = op.max_objects;
    g.covered = (unsigned *)T[FR_TRACK_COVERED];
    g.bits = (unsigned long long *)(scr + op.track_bits_offset);
    g.shift = (int *)T[FR_TRACK_SHIFT];
    g.S = op.track_shift; g.side = op.track_side; g.words = op.track_words; g.slabs = (int)op.track_slabs; g.track_maps = op.track_maps;
    g.p.f = a.f;
    g.p.L = (unsigned *)(scr + op.track_piece_offset); g.p.aux = g.p.L + op.track_maps * op.cells; g.p.rowcnt = g.p.aux + op.track_maps * op.cells;
    g.p.n_objects = (unsigned *)T[FR_TRACK_N]; g.p.table = (unsigned *)T[FR_TRACK_PIECES];
    g.p.n_maps = op.track_maps;
    g.p.connectivity = op.connectivity; g.p.min_area = 1; g.p.max_objects = op.track_pieces;
    HIPCHK(hipMemsetAsync(T[FR_TRACK_PIECES], 0, op.track_pieces_bytes, st));
    HIPCHK(hipMemsetAsync(T[FR_TRACK_COVERED], 0, op.track_covered_bytes, st));
    const dim3 thr(OBJ_THREADS);
    hipLaunchKernelGGL(k_track_bits, dim3((unsigned)op.grid_track_bits), thr, 0, st, g);
    HIPCHK(hipGetLastError());
    if (op.track_corr) {
        g.corr = op.track_corr_wanted ? (unsigned *)T[FR_TRACK_CORR] : (unsigned *)(scr + op.track_corr_offset);
        HIPCHK(hipMemsetAsync(g.corr, 0, op.track_corr_bytes, st));
        hipLaunchKernelGGL(k_track_corr, dim3((unsigned)op.grid_track_corr), thr, 0, st, g);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_track_shift, dim3((unsigned)op.grid_track_shift), thr, 0, st, g);
        HIPCHK(hipGetLastError());
    } else {
        // (checked by obj_check_track before anything was queued; the plan outlives the copy)
        HIPCHK(hipMemcpyAsync(g.shift, op.shifts_in.data(), op.track_shift_bytes, hipMemcpyHostToDevice, st));
    }
    const dim3 rows((unsigned)op.grid_track_rows);
    hipLaunchKernelGGL(k_track_runs, rows, thr, 0, st, g);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_merge, rows, thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_flatten, dim3((unsigned)op.grid_track_cells), thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_area, rows, thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_count, rows, thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_number, rows, thr, 0, st, g.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_track_attr, rows, thr, 0, st, g);
    HIPCHK(hipGetLastError());
    MatchArgs d{};
    d.p = g.p;
    hipLaunchKernelGGL(k_match_decode, dim3((unsigned)op.grid_track_decode), thr, 0, st, d);
    HIPCHK(hipGetLastError());
    return CPOL_OK;
}

// the kernels of cpol_obj.inl behind k_frac_score on `st`; fa: the maps as frac_launch resolved them
static int obj_launch(cpol_ctx *ctx, const FracArgs &fa, const FracPlan &pl, const ObjPlan &op, void *const T[FR_N], hipStream_t st)
{
    ENSURE(ctx->b_oscr, (size_t)op.scratch_bytes);
    ObjArgs a{};
    a.f = fa;
    a.L = (unsigned *)ctx->b_oscr.p; a.aux = a.L + op.n_maps * op.cells; a.rowcnt = a.aux + op.n_maps * op.cells;
    a.n_objects = (unsigned *)T[FR_OBJ_N]; a.table = (unsigned *)T[FR_OBJ_TABLE]; a.labels = op.labels ? (int *)T[FR_OBJ_LABELS] : nullptr;
    a.n_maps = op.n_maps;
    a.connectivity = op.connectivity; a.min_area = op.min_area; a.max_objects = op.max_objects;
    HIPCHK(hipMemsetAsync(T[FR_OBJ_TABLE], 0, op.table_bytes, st));
    const dim3 rows((unsigned)op.grid_rows), thr(OBJ_THREADS);
    hipLaunchKernelGGL(k_obj_runs, rows, thr, 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_merge, rows, thr, 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_flatten, dim3((unsigned)op.grid_cells), thr, 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_area, rows, thr, 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_count, rows, thr, 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_number, rows, thr, 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_attr, rows, thr, 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_obj_decode, dim3((unsigned)op.grid_decode), thr, 0, st, a);
    HIPCHK(hipGetLastError());
    if (op.sums) {
        const int rc = obj_launch_sums(ctx, a, op, T, st);
        if (rc != CPOL_OK) return rc;
    }
    if (op.match) {
        const int rc = obj_launch_match(ctx, a, op, T, st);
        if (rc != CPOL_OK) return rc;
    }
    return op.track ? obj_launch_track(ctx, a, op, T, st) : CPOL_OK;
}

// plane: block 0's plane on the device; obs_on_host: `observed` and `domain` are host arrays (copied to b_fobs on `st` first),
// else memory the device reads in place; T: where `sums` and `totals` (and the arrays of the objects and the probabilities) go
static int frac_launch(cpol_ctx *ctx, const cpol_fractions *f, const FracPlan &pl, const ObjPlan &op, const float *plane, long plane_stride,
                       bool obs_on_host, void *const T[FR_N], hipStream_t st)
{
    ENSURE(ctx->b_fsat, (size_t)pl.scratch_bytes);
    FracArgs a{};
    a.plane = plane; a.plane_stride = plane_stride;
    a.obs = f->observed; a.domain = f->domain;
    if (obs_on_host) {
        const size_t ob = ((size_t)pl.cells * sizeof(float) + 255) & ~(size_t)255;
        ENSURE(ctx->b_fobs, ob + (size_t)pl.cells);
        HIPCHK(hipMemcpyAsync(ctx->b_fobs.p, f->observed, (size_t)pl.cells * sizeof(float), hipMemcpyHostToDevice, st));
        a.obs = (const float *)ctx->b_fobs.p;
        if (f->domain) {
            HIPCHK(hipMemcpyAsync((char *)ctx->b_fobs.p + ob, f->domain, (size_t)pl.cells, hipMemcpyHostToDevice, st));
            a.domain = (const unsigned char *)ctx->b_fobs.p + ob;
        }
    }
    a.sat = (unsigned *)ctx->b_fsat.p;
    a.sums = (unsigned long long *)T[FR_SUMS]; a.totals = (unsigned long long *)T[FR_TOTALS];
    a.table = pl.table; a.n_blocks = pl.n_blocks;
    a.n_x = pl.n_x; a.n_y = pl.n_y; a.cells = (int)pl.cells;
    a.n_thr = pl.n_thr; a.n_radii = pl.n_radii;
    a.row_groups = (pl.n_y + FRAC_ROWS - 1) / FRAC_ROWS; a.col_chunks = pl.col_chunks; a.score_groups = pl.score_groups;
    for (int j = 0; j < pl.n_thr; ++j) a.thr[j] = pl.thr[j];
    for (int j = 0; j < pl.n_radii; ++j) a.radii[j] = pl.radii[j];
    HIPCHK(hipMemsetAsync(T[FR_SUMS], 0, pl.sums_bytes, st));
    HIPCHK(hipMemsetAsync(T[FR_TOTALS], 0, pl.totals_bytes, st));
    hipLaunchKernelGGL(k_frac_rows, dim3((unsigned)pl.grid_rows), dim3(FRAC_THREADS), 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_frac_cols, dim3((unsigned)pl.grid_cols), dim3(64), 0, st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_frac_score, dim3((unsigned)pl.grid_score), dim3(FRAC_THREADS), 0, st, a);
    HIPCHK(hipGetLastError());
    if (pl.prob.on) {              // the neighbourhood ensemble probabilities: one kernel on the finished tables
        const FracProbPlan &pp = pl.prob;
        FracProbArgs q{};
        q.f = a;
        q.prob_sums = (unsigned long long *)T[FR_PROB_SUMS]; q.reliability = (unsigned long long *)T[FR_RELIABILITY];
        q.member_sum = pp.member_sum ? (unsigned *)T[FR_MEMBER_SUM] : nullptr;
        q.member_any = pp.member_any ? (unsigned *)T[FR_MEMBER_ANY] : nullptr;
        q.n_members = (int)pl.n_blocks; q.table_entries = pp.table_entries;
        HIPCHK(hipMemsetAsync(q.prob_sums, 0, pp.prob_sums_bytes, st));
        HIPCHK(hipMemsetAsync(q.reliability, 0, pp.reliability_bytes, st));
        hipLaunchKernelGGL(k_frac_members, dim3((unsigned)pp.grid), dim3(FRAC_THREADS), 0, st, q);
        HIPCHK(hipGetLastError());
    }
    if (op.on) return obj_launch(ctx, a, pl, op, T, st);
    return CPOL_OK;
}

// The test hook cpol_debug_read "fractions_maps": the checks and the three kernels on caller-supplied maps (host memory in, host
// memory out, blocking) -- the kernels on maps no sweep produces (every value class, rows and columns across wavefront chunks,
// windows clipped at every border, the smallest and the longest grids).  f.objects rides the embedded struct, and with
// CPOL_FRAC_ENSEMBLE in f.n_radii the pointer behind f makes the two a cpol_fractions_ensemble: with them the object kernels and
// k_frac_members run on the same maps.
struct FracHook {
    int32_t n_blocks, n_y, n_x, pad_;
    const float *maps;                      // [n_blocks][n_y][n_x]
    cpol_fractions f;
};

static int frac_hook(cpol_ctx *ctx, const FracHook *hk)
{
    if (!hk->maps) { ctx->err = "fractions_maps: maps is NULL"; return CPOL_ERR_ARG; }
    FracPlan pl;
    const char *why = frac_check_maps(&hk->f, hk->n_x, hk->n_y, hk->n_blocks, &pl);
    if (why) { ctx->err = std::string("cpol_fractions: ") + why; return CPOL_ERR_ARG; }
    ObjPlan op;
    if ((why = obj_check(hk->f.objects, pl, &op)) != nullptr) { ctx->err = std::string("cpol_objects: ") + why; return CPOL_ERR_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = upload(ctx, ctx->b_fmaps, hk->maps, (size_t)pl.n_blocks * pl.cells * sizeof(float))) != CPOL_OK) return rc;
    PlaceArray arr[FR_N];
    frac_place(&hk->f, pl, op, arr);
    DevBuf *own[FR_N];
    for (int k = 0; k < FR_N; ++k) own[k] = &ctx->b_fout[k];
    return hook_finish(ctx, arr, own, [&](void *const *T) { return frac_launch(ctx, &hk->f, pl, op, (const float *)ctx->b_fmaps.p, pl.cells, true, T, ctx->stream); });
}

// The launch sequence of cpol_run_sweep, and its two halves:
// - cpol_run_columns (cols != NULL): k_columns_ingest copies the caller's sub-beam columns where k_interp_sweep would have
//   written the interpolated ones; `t` then holds the per-ray tables cpol_run_columns made of them, with one horizontal
//   and one vertical node per sub-beam and no ray paths;
// - cpol_interp_subbeams (sub_out != NULL): the sequence up to and including k_interp_sweep, then the geometry of every
//   sub-beam (k_interp_export), the 'ml' weights, the melting scheme and the copies to sub_out -- no scattering.
// - cpol_run_sweep_members (mem != NULL): a sweep of mem->n_members * mem->n_rays rays whose first half runs ONCE over
//   mem->n_rays rays (k_trajectory where the sweep would run it, then k_interp_members instead of k_interp_sweep) and writes
//   member mm into the rows [mm * mem->n_rays, ...) of the work arrays; `t` holds the per-ray tables repeated for every member.
//   The launch-form rules are the column call's: no interpolating forms, no graph replay.
//   With mem->timed (cpol_ray_tables_t.time_blend) the sweep keeps its n_rays rows: k_interp_timed writes ONE block of rows, the
//   values of ray r blended from mem->V[ray_state[r]] and the cube behind it; `t` is the caller's; the rest as above.
struct MembersCall {
    int n_members, n_rays;
    const float *V[CPOL_MEMBERS_PER_CALL];
    bool timed;
    const int32_t *ray_state;           // [n_rays] host (timed)
    const float *ray_weight;            // [n_rays] host (timed)
};

// the next slot of the page-locked staging ring, grown to `bytes`; its last copy has left the buffer (t_free: when that was known)
static int staging_slot(cpol_ctx *ctx, size_t bytes, cpol_ctx::Staging **slot, double *t_free = nullptr)
{
    cpol_ctx::Staging &sg = ctx->stg[ctx->stg_next];
    ctx->stg_next = (ctx->stg_next + 1) % 4;
    if (sg.used) HIPCHK(hipEventSynchronize(sg.ev));
    if (t_free) *t_free = now_ns();
    if (sg.cap < bytes) {
        if (sg.p) (void)hipHostFree(sg.p);
        sg.p = nullptr; sg.cap = 0;
        HIPCHK(hipHostMalloc(&sg.p, bytes + bytes / 4 + 4096, hipHostMallocDefault));
        sg.cap = bytes + bytes / 4 + 4096;
    }
    if (!sg.ev) HIPCHK(hipEventCreateWithFlags(&sg.ev, hipEventDisableTiming));
    *slot = &sg;
    return CPOL_OK;
}

static int run_sequence(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_ray_tables_t *t,
                        const cpol_columns_t *cols, cpol_subbeam_outputs *sub_out, cpol_outputs *out,
                        const MembersCall *mem = nullptr)
{
    if (!ctx) return CPOL_ERR_ARG;
    if (!p || !t || !out || !(ctx->model_staged || cols) || ctx->hs.n_hydro < 1 || p->n_rays < 1 ||
        p->n_gates < 1 || p->n_sub < 1 || p->n_hnodes < 1 || p->n_vnodes < 1 || (!t->traj && !cols) ||
        !t->geo || !t->sub_h || !t->sub_v || !t->sub_w) {
        ctx->err = "cpol_run_sweep: model / hydrometeors not staged or bad arguments";
        return CPOL_ERR_ARG;
    }
    if (t->time_blend != 0 && !(mem && mem->timed)) {
        ctx->err = "cpol_ray_tables_t.time_blend belongs to cpol_run_sweep_members alone";
        return CPOL_ERR_ARG;
    }
    const bool timed = mem && mem->timed;
    const double t_enter = now_ns();
    (void)hipGetLastError();            // a stale error of another user of the runtime in this thread is not ours
    for (int j = 0; j < ctx->hs.n_hydro; ++j)
        if (!ctx->hydro_staged[j]) { ctx->err = "cpol_run_sweep: hydrometeor slot not staged"; return CPOL_ERR_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->parent && ctx->itab_serial != ctx->lut_serial) {
        const int rc_it = build_itabs(ctx);                // once per staged table set
        if (rc_it != CPOL_OK) return rc_it;
    }
    hipStream_t st = ctx->stream;
    const int n_rays = p->n_rays, ng = p->n_gates, n_sub = p->n_sub;
    const int n_h = p->n_hnodes, n_v = p->n_vnodes;
    const int n_vars = cols ? cols->n_vars : ctx->model.n_vars, n_hyd = ctx->hs.n_hydro, n_keys = ctx->hs.n_keys;
    const long n_rg = (long)n_rays * ng;
    const long n_sbg = n_rg * n_sub;
    const int geo_rays = mem ? mem->n_rays : n_rays;     // the rays the geometry is evaluated for (ensemble: once for all members; timed: n_rays)
    if (n_sbg >= (1L << 31)) { ctx->err = "cpol_run_sweep: too many sub-beam gates in one call"; return CPOL_ERR_ARG; }
    {
        // re-validated here: a C caller may have reached this state through cpol_stage_hydro alone
        long total = 0;
        for (int j = 0; j < n_hyd; ++j) total += (long)ctx->hs.h[j].d.n_e * ctx->hs.h[j].d.n_t;
        if (total != n_keys || n_keys > 1024 * CPOL_SCAN_MAX_PER) {
            ctx->err = "cpol_run_sweep: inconsistent / too many LUT slices for the bucket scan (restage the hydrometeors)";
            return CPOL_ERR_ARG;
        }
        if ((long)n_rays * n_sub >= (1L << 31) || cdiv(ng, 256) > 65535 || p->outputs_on_device < 0 ||
            p->outputs_on_device > 2) {
            ctx->err = "cpol_run_sweep: launch-grid limits exceeded (n_rays * n_sub < 2^31, n_gates <= 65535 * 256) or bad outputs_on_device";
            return CPOL_ERR_ARG;
        }
        // (refused here, before the table uploads and the geometry kernel are queued: nothing of the call has reached the device)
        if (ng > CPOL_MAX_GATES) {
            ctx->err = "cpol_run_sweep: n_gates too large for the range scans (3 * n_gates floats of LDS: at most CPOL_MAX_GATES gates)";
            return CPOL_ERR_ARG;
        }
    }
    // every output array of the call, for the placement plan (cpol_place.h): the sweep's own, then those of the call's ONE product
    // (cpol_products.h) in the one slot range behind them, the fractions' behind the composite's
    enum { O_ZH, O_ZV, O_ZDR, O_KDP, O_DHV, O_PHIDP, O_RHOHV, O_ATTH, O_ATTV, O_MASK, O_LAT, O_LON,
           O_DIST, O_HGT, O_RVEL, O_MODEL, O_SZT, O_SPEC, O_MASK8, O_VIS, O_N, A_PR = O_N,
           PR_MAX = std::max({(int)SO_N, (int)MS_N, (int)SM_N, (int)CPOL_HIST_FIELDS, (int)CP_N + (int)FR_N, (int)SP_N}), A_N = A_PR + PR_MAX };
    static_assert(A_N <= PLACE_MAX_ARRAYS, "cpol_place.h: PLACE_MAX_ARRAYS");
    PlaceArray arr[A_N];
    DevBuf *own[A_N] = {};         // outside the window image and the caller's device memory every array of the sweep keeps a grow-only buffer of its own
    // the product and every refusal of it here, before anything of the call is queued
    const CallProduct cq = call_product(cols ? CALL_COLUMNS : timed ? CALL_TIMED : mem ? CALL_MEMBERS : CALL_SWEEP, *out);
    if (cq.refuse) { ctx->err = cq.refuse; return CPOL_ERR_ARG; }
    const cpol_superob *const so = out->superob;
    const cpol_member_stats *const ms = out->member_stats;
    const cpol_member_verify *const mv = out->member_verify;        // (the verification of the pass)
    const cpol_spectrum_moments *const sm = out->spectrum_moments;
    const cpol_histogram *const hg = out->histogram;
    const cpol_composite *const cp = out->composite;
    const cpol_fractions *const fr = out->fractions;                // (the neighbourhood verification of the composite)
    const cpol_species *const sp = out->species;
    SuperobPlan so_pl{};
    MemberStatsPlan ms_pl{};
    HistPlan hg_pl;
    CompPlan &cp_pl = ctx->cplan;
    FracPlan &fr_pl = ctx->fplan;
    ObjPlan &ob_pl = ctx->oplan;
    int rc = CPOL_OK;
    switch (cq.product) {          // (the superobservations and the statistics are packed into their blocks; the others are arrays of the sweep)
    case PRODUCT_SUPEROB: rc = superob_plan(ctx, so, n_rays, geo_rays, ng, p->simulate_doppler != 0, &so_pl, arr + A_PR); break;
    case PRODUCT_MEMBER_STATS:
        rc = member_stats_plan(ctx, ms, mv, (long)geo_rays * ng, n_rays / geo_rays, p->simulate_doppler != 0, &ms_pl, arr + A_PR);
        break;
    case PRODUCT_SPECTRUM_MOMENTS:
        rc = spec_moments_plan(ctx, sm, n_rg, p->simulate_doppler == 3, arr + A_PR);
        own[A_PR + SM_MOMENTS] = &ctx->b_smom; own[A_PR + SM_COUNT] = &ctx->b_smcount;
        break;
    case PRODUCT_HISTOGRAM: {
        HistCall hc;
        hc.n_rows = n_rays; hc.n_gates = ng; hc.doppler = p->simulate_doppler != 0;
        hc.n_model_vars = p->integrate_model ? n_vars : 0;
        rc = hist_plan(ctx, hg, hc, &hg_pl, arr + A_PR);
        for (int k = 0; k < CPOL_HIST_FIELDS; ++k) own[A_PR + k] = &ctx->b_hcounts[k];     // (a finishing call's counts)
        break;
    }
    case PRODUCT_COMPOSITE: {
        CompCall cc;
        cc.n_rows = n_rays; cc.n_gates = ng;
        cc.spaceborne = t->site != nullptr || p->geometry_mode == CPOL_GEOM_SPACEBORNE;
        for (int k = 0; k < CP_N; ++k) own[A_PR + k] = &ctx->b_cout[k];                     // (a finishing call's maps, and their scores)
        for (int k = 0; k < FR_N; ++k) own[A_PR + CP_N + k] = &ctx->b_fout[k];
        if ((rc = comp_plan(ctx, cp, cc, &cp_pl, arr + A_PR)) != CPOL_OK || !fr) break;
        // against the composite's plan, which passed; the object cells (cpol_objects) against the fractions' plan, which passed
        const char *why = frac_check(fr, cp, &cp_pl, &fr_pl);
        if (why) { ctx->err = std::string("cpol_fractions: ") + why; return CPOL_ERR_ARG; }
        if ((why = obj_check(fr->objects, fr_pl, &ob_pl)) != nullptr) { ctx->err = std::string("cpol_objects: ") + why; return CPOL_ERR_ARG; }
        frac_place(fr, fr_pl, ob_pl, arr + A_PR + CP_N);
        break;
    }
    case PRODUCT_SPECIES:
        rc = species_plan(ctx, sp, n_rg, n_hyd, arr + A_PR);
        for (int k = 0; k < SP_N; ++k) own[A_PR + k] = &ctx->b_spout[k];
        break;
    }
    if (rc != CPOL_OK) return rc;
    if (cq.refuse_after_plan) { ctx->err = cq.refuse_after_plan; return CPOL_ERR_ARG; }

    // ---- per-sweep host tables -> device (skipped when the caller's tag is unchanged) ----
    const int mode = p->geometry_mode;
    if ((mode == CPOL_GEOM_SPACEBORNE && !t->site) || (mode == CPOL_GEOM_HOST_PATHS && !t->paths) ||
        mode < 0 || mode > 2) {
        ctx->err = "cpol_run_sweep: geometry_mode needs tables->site (spaceborne) / tables->paths (host paths)";
        return CPOL_ERR_ARG;
    }
    const bool cut = p->apply_sensitivity && t->sens_thr;
    // integration scheme 'ml': per-gate weights, made by k_ml_weights (sweeps) or supplied with the columns
    const bool ml = cols ? cols->wgate != nullptr : t->sub_smooth != nullptr;
    const bool ml_tab = ml && !cols;
    const bool melt_given = cols && cols->q_melt;       // columns with the caller's melting fields
    if (ml_tab && (!t->ml_filter || t->ml_radius < 0 || t->ml_radius > 64)) {
        ctx->err = "cpol_run_sweep: sub_smooth needs ml_filter / ml_radius";
        return CPOL_ERR_ARG;
    }
    // terrain shadowing and the visibility (include/cosmo_pol_amd.h, "Terrain shadowing"): refused here, with nothing queued
    if (p->terrain_shadow != 0 && p->terrain_shadow != 1) { ctx->err = "cpol_run_sweep: terrain_shadow is 0 or 1"; return CPOL_ERR_ARG; }
    const bool shadow = p->terrain_shadow == 1;
    if (shadow && cols) {
        ctx->err = "cpol_run_columns: terrain_shadow is not taken: the caller's masks stand (shadow them first, cosmo_pol_amd/shadow.py)";
        return CPOL_ERR_ARG;
    }
    if (shadow && (t->site || mode == CPOL_GEOM_SPACEBORNE)) {
        ctx->err = "cpol_run_sweep: terrain_shadow is not taken with spaceborne geometry (the gates of a swath run from the satellite downward)";
        return CPOL_ERR_ARG;
    }
    if (out->visibility && ml) {
        ctx->err = "cpol_run_sweep: outputs->visibility is not defined with per-gate weights (integration scheme 'ml')";
        return CPOL_ERR_ARG;
    }
    // (k_terrain_shadow's grid, a quarter of the n_rays * n_sub rows, stays below 2^31: the launch-grid limits above refuse more)
    const long shape[6] = {n_rays, ng, n_sub, n_h, n_v, (ml_tab ? 64 + t->ml_radius * 128L : 0) + (long)mode * 8 + (t->nyquist ? 4 : 0) + (t->site ? 2 : 0) + (cut ? 1 : 0)
                           + (t->varray ? 16 + p->n_vbins * 65536L : 0)};
    void **const views[11] = {&ctx->v_traj_in, &ctx->v_site, &ctx->v_geo, &ctx->v_subh, &ctx->v_subv, &ctx->v_subw,
                              &ctx->v_sens, &ctx->v_nyq, &ctx->v_subsmooth, &ctx->v_mlfilter, &ctx->v_varray};
    cpol_ctx::TableSet *set = nullptr, *lru = &ctx->tsets[0];
    for (auto &ts : ctx->tsets) {
        if (t->version != 0 && ts.version == t->version && memcmp(shape, ts.shape, sizeof shape) == 0) set = &ts;
        if (ts.last_use < lru->last_use) lru = &ts;
    }
    const bool reuse = set != nullptr;
    if (!set) set = lru;
    // which kernels this call launches and in which form: every rule in cpol_forms.h, decided here once
    FormIn fi;
    fi.n_rays = n_rays; fi.n_gates = ng; fi.n_sub = n_sub; fi.n_h = n_h; fi.geo_rays = geo_rays;
    fi.columns = cols != nullptr; fi.sub_export = sub_out != nullptr; fi.members = mem != nullptr; fi.timed = timed;
    fi.melt_given = melt_given; fi.ml = ml; fi.skip_melting = sub_out && sub_out->skip_melting;
    fi.geometry_mode = mode; fi.doppler = p->simulate_doppler;
    fi.site = t->site != nullptr; fi.versioned = t->version != 0; fi.with_melting = p->with_melting != 0;
    fi.exact_sub = (p->debug_flags & CPOL_DEBUG_EXACT_SUBBEAMS) != 0;
    fi.want_latlon = out->lats || out->lons; fi.want_sz_total = out->sz_total != nullptr;
    // (a histogram over a model variable: the model variables are integrated as if they had been asked for)
    fi.want_model = p->integrate_model && (out->model_vars || (hg && hg->ordinate >= HIST_ORD_MODEL)); fi.reuse = reuse;
    fi.outputs_on_device = p->outputs_on_device;
    fi.keep_debug = ctx->keep_debug; fi.timing = ctx->timing; fi.nz = ctx->model.nz;
    fi.lanes = ctx->parent ? ctx->parent->n_children : ctx->n_children;
    fi.scan_form = CPOL_SCAN_FORM;
    fi.shadow = shadow;
    fi.want_species = cq.product == PRODUCT_SPECIES;       // (the general launch sequence: it alone forms the per-species rows)
    fi.n_hydro = n_hyd;
    for (int j = 0; j < n_hyd; ++j) {
        const cpol_hydro_desc &d = ctx->hs.h[j].d;
        const ItabDev &tj = ctx->its.t[j];
        FormSpecies &s = fi.s[j];
        s.tab = tj.tab != nullptr; s.two_d = tj.two_d != 0; s.writes_vn = tj.writes_vn != 0;
        s.pan_lo = tj.pan_lo; s.pan_hi = tj.pan_hi; s.n_pan = tj.n_pan;
        s.psd_family = d.psd_family; s.numeric_intv = d.numeric_intv; s.q_source = d.q_source; s.uniform_grid = d.uniform_grid;
        s.tab_degree = d.tab_degree; s.rule = d.rule; s.var_q = d.var_q;
        s.pre = ctx->hs.h[j].pre != nullptr; s.dnu = ctx->hs.h[j].dnu != nullptr;
    }
    const ProcessKnobs &pk = process_knobs();
    const Forms f = choose_forms(fi, ctx->knobs, pk);
    // ---- the remaining refusals: every argument check of the call happens here, before a table set or a staging slot is taken
    // and before anything is queued -- a refused call leaves nothing on the device and the context as it found it ----
    const bool doppler = p->simulate_doppler != 0;
    const bool dop2 = p->simulate_doppler == 2;
    const bool dop3 = p->simulate_doppler == 3;
    const int n_vb = p->n_vbins;
    bool spec_melt = false;                // Doppler scheme 3: a melting species is staged (its fall-speed tables take LDS of k_spec_gate)
    size_t spec_lds = 0;                   // ... and the LDS of a workgroup of k_spec_gate
    if (dop3) {
        if (n_vb < 2 || n_vb > 4097 || !t->varray || p->var_rho < 0 || p->var_rho >= n_vars) {
            ctx->err = "cpol_run_sweep: Doppler scheme 3 needs n_vbins in [2, 4097], tables->varray and var_rho";
            return CPOL_ERR_ARG;
        }
        for (int j = 0; j < n_hyd; ++j) {
            if (!ctx->ss.s[j].rcs32) { ctx->err = "cpol_run_sweep: Doppler scheme 3 needs cpol_stage_spectrum_tables"; return CPOL_ERR_ARG; }
            if (ctx->hs.h[j].d.n_d != ctx->hs.h[0].d.n_d) {     // the LDS image is sized from slot 0
                ctx->err = "cpol_run_sweep: Doppler scheme 3 needs the same number of diameter bins in every table";
                return CPOL_ERR_ARG;
            }
        }
        for (int j = 0; j < n_hyd; ++j) spec_melt = spec_melt || ctx->hs.h[j].d.psd_family == CPOL_PSD_MELTING;
        // [2][n_d] + [threads] float64 (only with melting species), [n_hyd][n_d] + [n_hyd + 1][n_v] float32 (cpol_spectrum.inl)
        spec_lds = (spec_melt ? ((size_t)2 * ctx->hs.h[0].d.n_d + CPOL_SPEC_THREADS) * sizeof(double) : 0)
                   + ((size_t)n_hyd * (ctx->hs.h[0].d.n_d + n_vb) + n_vb) * sizeof(float);
        if (spec_lds > 160 * 1024 - 256) {
            // (gfx950: 160 KB of LDS per CU, all of it available to ONE workgroup of k_spec_gate when the launch asks for it --
            // six species with FFT_length = 2048, the upper end of the reference's valid range (cfg.py:91), need 100 KB)
            ctx->err = "cpol_run_sweep: Doppler scheme 3: n_hydro x (n_d + n_vbins) exceeds the 160 KB of LDS of a gfx950 CU";
            return CPOL_ERR_ARG;
        }
    }
    const bool broaden = p->turbulence_correction != 0 || p->motion_correction != 0;
    if (broaden) {
        if (!dop3) { ctx->err = "cpol_run_sweep: turbulence_correction / motion_correction need Doppler scheme 3"; return CPOL_ERR_ARG; }
        if (p->turbulence_correction && (p->var_edr < 0 || p->var_edr >= n_vars)) {
            ctx->err = "cpol_run_sweep: turbulence_correction needs var_edr, the staged index of the eddy dissipation rate";
            return CPOL_ERR_ARG;
        }
        if (!(p->v_res > 0.0) || (p->turbulence_correction && (!(p->sigma_r > 0.0) || !(p->sigma_theta > 0.0))) ||
            (p->motion_correction && !(p->motion_den > 0.0))) {
            ctx->err = "cpol_run_sweep: spectrum broadening needs v_res > 0, sigma_r, sigma_theta > 0 (turbulence), motion_den > 0 (motion)";
            return CPOL_ERR_ARG;
        }
    }
    if (dop2)
        for (int j = 0; j < n_hyd; ++j)
            if (!ctx->hs.h[j].rcsw) { ctx->err = "cpol_run_sweep: Doppler scheme 2 needs cpol_stage_doppler_weights"; return CPOL_ERR_ARG; }
    if (out->mask_sum8 && 2 * n_sub > 127) { ctx->err = "cpol_run_sweep: outputs->mask_sum8 needs 2 * n_sub <= 127 (one byte per gate)"; return CPOL_ERR_ARG; }
    const bool melt_vars = f.melt_qr >= 0 && f.melt_qs >= 0 && f.melt_qg >= 0;      // 1-moment rain, snow and graupel slots are staged
    if (sub_out && p->with_melting && !melt_vars) {
        ctx->err = "cpol_interp_subbeams: melting needs 1-moment rain, snow and graupel slots";
        return CPOL_ERR_ARG;
    }
    if (!sub_out) {                        // (the export stops before the kernels that read these)
        if (doppler && (p->var_u < 0 || p->var_v < 0 || p->var_w < 0 || p->var_u >= n_vars || p->var_v >= n_vars || p->var_w >= n_vars)) {
            ctx->err = "cpol_run_sweep: simulate_doppler needs var_u / var_v / var_w";
            return CPOL_ERR_ARG;
        }
        if (p->with_melting && !melt_vars) {
            ctx->err = "cpol_run_sweep: melting needs 1-moment rain, snow and graupel slots";
            return CPOL_ERR_ARG;
        }
    }
    if (spec_lds > 64 * 1024) {
        // beyond the default 64 KB per workgroup: ask for it (an attribute of the kernel; the largest request so far is kept)
        cpol_ctx *const root = root_of(ctx);
        if (spec_lds > root->spec_lds_allowed) {
            HIPCHK(hipFuncSetAttribute((const void *)k_spec_gate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)spec_lds));
            root->spec_lds_allowed = spec_lds;
        }
    }
    set->last_use = ++ctx->tset_clock;
    if (reuse) {
        for (int k = 0; k < 11; ++k) *views[k] = set->views[k];
    } else {
        // pack every table of this sweep into one pinned staging slot, one H2D copy
        struct Item { const void *src; size_t bytes; };
        const Item items[11] = {
            {t->traj, t->traj ? (size_t)n_rays * n_v * CPOL_TRAJ_STRIDE * sizeof(double) : 0},
            {t->site, t->site ? (size_t)n_rays * CPOL_SITE_STRIDE * sizeof(double) : 0},
            {t->geo, (size_t)n_rays * n_h * CPOL_GEO_STRIDE * sizeof(double)},
            {t->sub_h, (size_t)n_sub * sizeof(int)},
            {t->sub_v, (size_t)n_sub * sizeof(int)},
            {t->sub_w, (size_t)n_sub * sizeof(double)},
            {cut ? t->sens_thr : nullptr, cut ? (size_t)ng * sizeof(double) : 0},
            {t->nyquist, t->nyquist ? (size_t)n_rays * sizeof(double) : 0},
            {ml_tab ? t->sub_smooth : nullptr, ml_tab ? (size_t)n_sub * sizeof(int) : 0},
            {ml_tab ? t->ml_filter : nullptr, ml_tab ? (size_t)(2 * t->ml_radius + 1) * sizeof(double) : 0},
            {t->varray, t->varray ? (size_t)p->n_vbins * sizeof(double) : 0},
        };
        size_t total = 0;
        for (const Item &it : items) total += (it.bytes + 63) & ~(size_t)63;
        set->version = 0;                                        // (not valid until the copy is queued)
        set->poly_version = 0;                                   // (other rays: their polynomials are made again)
        ENSURE(set->buf, total);
        cpol_ctx::Staging *sgp = nullptr;
        const double t_s0 = now_ns();
        double t_s1 = t_s0;
        if ((rc = staging_slot(ctx, total, &sgp, &t_s1)) != CPOL_OK) return rc;
        cpol_ctx::Staging &sg = *sgp;
        size_t off = 0;
        for (int k = 0; k < 11; ++k) {
            const Item &it = items[k];
            set->views[k] = it.bytes ? (void *)((char *)set->buf.p + off) : nullptr;
            *views[k] = set->views[k];
            if (it.bytes) memcpy((char *)sg.p + off, it.src, it.bytes);
            off += (it.bytes + 63) & ~(size_t)63;
        }
        const double t_s2 = now_ns();
        if (ctx->knobs.upload_kernel) {
            const long n16 = (long)(total / 16);          // (every table is padded to 64 bytes)
            hipLaunchKernelGGL(k_upload_tables, dim3((unsigned)std::min<long>(cdiv(n16, 256), 256)), dim3(256), 0, ctx->stream,
                               (uint4 *)set->buf.p, (const uint4 *)sg.p, n16);
        } else {
            HIPCHK(hipMemcpyAsync(set->buf.p, sg.p, total, hipMemcpyHostToDevice, ctx->stream));
        }
        const double t_s3 = now_ns();
        HIPCHK(hipEventRecord(sg.ev, ctx->stream));
        const double t_s4 = now_ns();
        ctx->host_ns[6] += t_s1 - t_s0; ctx->host_ns[7] += t_s2 - t_s1; ctx->host_ns[8] += t_s3 - t_s2; ctx->host_ns[9] += t_s4 - t_s3;
        sg.used = true;
        set->version = t->version;
        memcpy(set->shape, shape, sizeof shape);
    }
    const double t_tables = now_ns();
    // ---- work buffers: which, and how large, is decided in cpol_buffers.h; every allocation of the sequence happens here, before
    // anything of the call is queued, like every argument check above (an error return further down would leave the sweep's
    // counter set half used; see counters_dirty) ----
    BufIn bi;
    bi.n_rays = n_rays; bi.n_gates = ng; bi.n_sub = n_sub; bi.n_h = n_h; bi.n_v = n_v; bi.n_vars = n_vars; bi.n_hydro = n_hyd;
    bi.n_keys = n_keys; bi.n_vbins = n_vb; bi.mode = mode;
    bi.keep_debug = ctx->keep_debug; bi.ml = ml; bi.doppler = doppler; bi.dop3 = dop3; bi.broaden = broaden; bi.timed = timed;
    bi.sub_export = sub_out != nullptr;
    bi.want_species = fi.want_species;
    bi.classify_threads = CPOL_CLASSIFY_THREADS; bi.present_words = CPOL_GATE1_PRESENT != 0;
    bi.f = f;
    // columns: where k_columns_ingest reads each input (host inputs: a device staging area, one copy per array)
    const void *col_src[BUF_MAX_COLS] = {};
    if (cols) {
        const void *const rest[6] = {cols->mask, cols->elev, ml ? cols->wgate : nullptr, melt_given ? cols->q_melt : nullptr,
                                     melt_given ? cols->fw_melt : nullptr, melt_given ? cols->has_melting : nullptr};
        for (int v = 0; v < n_vars; ++v) col_src[v] = cols->vals[v];
        for (int k = 0; k < 6; ++k) { col_src[n_vars + k] = rest[k]; bi.col_given[k] = rest[k] != nullptr; }
        bi.columns = true; bi.inputs_on_device = cols->inputs_on_device != 0;
    }
    const BufPlan bp = plan_buffers(bi);
    const long cnt_stride = bp.cnt_stride, unit_cap = bp.unit_cap;
    const bool was_dirty = ctx->counters_dirty;          // (the previous sequence was cut short: its rays' tickets may be half taken too)
    // (a buffer the plan gives 0 bytes is not touched; of the buffers a call always needs none can come out at 0: the argument
    // checks above refuse n_rays, n_gates, n_sub < 1, and n_keys is the sum of n_e * n_t over at least one staged species)
    bool replaced[WB_N] = {};
    for (int w = 0; w < WB_N; ++w) {
        if (!bp.bytes[w]) continue;
        DevBuf &b = ctx->*WORK_BUFS[w];
        void *const was = b.p;
        ENSURE(b, bp.bytes[w]);
        replaced[w] = b.p != was;
    }
    // the fills of a replaced buffer (BufRow::fill), over its whole capacity; the two counter sets together, over what the call
    // uses, also when the stride changed or the previous call returned an error after its counting kernel was queued
    // (counters_dirty -- a failed copy or capture: its set holds counts and the serial did not advance, so the set would be used
    // again as it is; the memsets are queued behind whatever that call left on the stream)
    const bool clear_counters = replaced[WB_COUNT] || replaced[WB_TOTALS] || ctx->count_stride != cnt_stride || ctx->counters_dirty;
    for (int w = 0; w < WB_N; ++w) {
        if (!bp.bytes[w] || BUF_ROWS[w].fill == FILL_NONE) continue;
        const bool counter = w == WB_COUNT || w == WB_TOTALS;
        if (!(counter ? clear_counters : replaced[w] || (w == WB_TICKET && was_dirty))) continue;
        const DevBuf &b = ctx->*WORK_BUFS[w];
        HIPCHK(hipMemsetAsync(b.p, BUF_ROWS[w].fill == FILL_FF ? 0xFF : 0, counter ? bp.bytes[w] : b.cap, ctx->stream));
    }
    if (clear_counters) { ctx->count_stride = cnt_stride; ctx->counters_dirty = false; }
    const int par = (int)(ctx->sweep_serial & 1);        // (the serial advances once the sequence is queued)
    int *const cnt_p = (int *)ctx->b_count.p + par * cnt_stride, *const cnt_next = (int *)ctx->b_count.p + (par ^ 1) * cnt_stride;
    long long *const tot_p = (long long *)ctx->b_totals.p + par * 4, *const tot_next = (long long *)ctx->b_totals.p + (par ^ 1) * 4;
    // arc distance <= slant range; a margin of 1e-3 for the asin of the 4/3-earth formula
    const double geo_poly_scale = 2.0 / ((p->range0 + (double)(ng - 1) * p->range_step) * 1.001);
    if (f.geo_poly || f.poly_single) {
        if (!ctx->d_geoM.p) {
            // Chebyshev-node values -> monomial coefficients (as build_itabs' M), extended precision on the host
            constexpr int NP = CPOL_GEO_NP;
            long double T[NP][NP] = {};
            T[0][0] = 1.0L;
            if (NP > 1) T[1][1] = 1.0L;
            for (int k = 2; k < NP; ++k)
                for (int pw = 0; pw < NP; ++pw) T[k][pw] = (pw > 0 ? 2.0L * T[k - 1][pw - 1] : 0.0L) - T[k - 2][pw];
            const long double pi = 3.141592653589793238462643383279502884L;
            double M[NP * NP];
            for (int pw = 0; pw < NP; ++pw)
                for (int q = 0; q < NP; ++q) {
                    long double acc = 0.0L;
                    for (int k = 0; k < NP; ++k) acc += T[k][pw] * (k == 0 ? 1.0L : 2.0L) / NP * cosl(pi * k * (q + 0.5L) / NP);
                    M[pw * NP + q] = (double)acc;
                }
            rc = upload(ctx, ctx->d_geoM, M, sizeof M);
            if (rc != CPOL_OK) return rc;
            HIPCHK(hipStreamSynchronize(ctx->stream));           // (M is a stack array)
        }
        if (f.poly_single && (!set->poly.p || set->poly_version != set->version || set->poly_scale != geo_poly_scale ||
                            set->poly_site[0] != p->radar_lon || set->poly_site[1] != p->sin_u1 || set->poly_site[2] != p->cos_u1)) {
            ENSURE(set->poly, (size_t)n_rays * n_h * 2 * CPOL_GEO_NP * sizeof(double));
            TrajArgs tp{};
            tp.geo = (const double *)ctx->v_geo;
            tp.n_rays = geo_rays; tp.n_h = n_h; tp.n_v = n_v; tp.n_gates = ng; tp.mode = mode;
            tp.lon1 = p->radar_lon; tp.sin_u1 = p->sin_u1; tp.cos_u1 = p->cos_u1;
            tp.poly = (double *)set->poly.p;
            tp.poly_M = (const double *)ctx->d_geoM.p;
            tp.poly_scale = geo_poly_scale;
            hipLaunchKernelGGL(k_trajectory, dim3((unsigned)cdiv((long)geo_rays * n_h, 256 / CPOL_GEO_NP)), dim3(256), 0, ctx->stream, ctx->model, tp);
            set->poly_version = set->version;
            set->poly_scale = geo_poly_scale;
            set->poly_site[0] = p->radar_lon; set->poly_site[1] = p->sin_u1; set->poly_site[2] = p->cos_u1;
        }
    }
    if (timed) {
        // the per-ray brackets: through a slot of the page-locked staging ring (a copy from the caller's pageable arrays would make the
        // call wait for the stream), one host-to-device copy, skipped when the context's device copy already holds these values
        const size_t nb = (size_t)n_rays * sizeof(int32_t), total = 2 * nb;
        if (replaced[WB_TIMED]) ctx->timed_shadow.clear();
        if (ctx->timed_shadow.size() != total || memcmp(ctx->timed_shadow.data(), mem->ray_state, nb) != 0 ||
            memcmp(ctx->timed_shadow.data() + nb, mem->ray_weight, nb) != 0) {
            ctx->timed_shadow.clear();                           // (not valid until the copy is queued)
            cpol_ctx::Staging *sgp = nullptr;
            if ((rc = staging_slot(ctx, total, &sgp)) != CPOL_OK) return rc;
            cpol_ctx::Staging &sg = *sgp;
            memcpy(sg.p, mem->ray_state, nb);
            memcpy((char *)sg.p + nb, mem->ray_weight, nb);
            HIPCHK(hipMemcpyAsync(ctx->b_timed.p, sg.p, total, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipEventRecord(sg.ev, ctx->stream));
            sg.used = true;
            try {
                ctx->timed_shadow.assign((const char *)sg.p, (const char *)sg.p + total);
            } catch (...) { ctx->timed_shadow.clear(); }
        }
    }
    // ---- outputs: where the kernels write each array, and how it reaches the caller ----
    const bool dev = p->outputs_on_device == 1;
    const bool async_host = p->outputs_on_device == 2;    // pinned host buffers, no wait
    const bool want_szt = f.want_szt, want_model = fi.want_model;
    // the float32 constants of the final stage, c_zh, c_kdp, c_2w: FinalArgs takes them, and so does k_species behind the sequence
    const float fa_c[3] = {(float)p->c_zh, (float)(1e-3 * (180.0 / 3.14159265358979323846) * p->wavelength), (float)(2 * p->wavelength)};
    void *const user_out[O_N] = {out->ZH, out->ZV, out->ZDR, out->KDP, out->DELTA_HV, out->PHIDP,
                                 out->RHOHV, out->ATT_H, out->ATT_V, out->mask, out->lats, out->lons,
                                 out->dist, out->heights, out->RVEL, out->model_vars, out->sz_total,
                                 out->DSPECTRUM, out->mask_sum8, out->visibility};
    constexpr int N_OUT = (int)(sizeof ctx->b_out / sizeof ctx->b_out[0]);      // (the arrays behind O_HGT have buffers of their own names, below)
    static_assert(N_OUT > O_HGT && N_OUT <= O_N, "b_out: a buffer for each of the first fourteen arrays");
    for (int k = 0; k < O_N; ++k) arr[k].user = (uintptr_t)user_out[k];
    for (int k = 0; k < N_OUT; ++k) own[k] = &ctx->b_out[k];
    for (int k = 0; k < 14; ++k) {
        arr[k].bytes = (size_t)n_rg * ((k == O_MASK || k == O_LAT || k == O_LON) ? sizeof(double) : sizeof(float));
        arr[k].produced = !(cols && k >= O_LAT && k <= O_HGT);      // (the columns carry no gate coordinates)
        if (mem && !timed && k >= O_LAT && k <= O_HGT) arr[k].bytes = arr[k].bytes / (size_t)mem->n_members;      // (the geometry once, not per member)
    }
    arr[O_RVEL].bytes = (size_t)n_rg * sizeof(double);            arr[O_RVEL].produced = doppler;     own[O_RVEL] = &ctx->b_rvel;
    arr[O_MODEL].bytes = (size_t)n_vars * n_rg * sizeof(double);  arr[O_MODEL].produced = want_model; own[O_MODEL] = &ctx->b_model;
    arr[O_SZT].bytes = (size_t)n_rg * CPOL_N_SZ * sizeof(float);  arr[O_SZT].produced = want_szt;     own[O_SZT] = &ctx->b_sztotal;
    arr[O_SZT].own_under_debug = true;                            // (cpol_debug_read "sz_total" reads the context's copy)
    arr[O_SPEC].bytes = (size_t)n_rg * n_vb * sizeof(double);     arr[O_SPEC].produced = dop3;        own[O_SPEC] = &ctx->b_spectrum;
    // the radial mask as one byte per gate (the sum of the sub-beams' codes): only when asked for; the float64 form is then
    // written only if it is asked for too
    arr[O_MASK8].bytes = (size_t)n_rg;                            arr[O_MASK8].produced = out->mask_sum8 != nullptr; own[O_MASK8] = &ctx->b_mask8;
    if (out->mask_sum8 && !out->mask && !ctx->keep_debug) arr[O_MASK].produced = false;
    // the visible share of the antenna pattern: geometry rows only (an ensemble call: once, like the gate coordinates); only when asked for
    arr[O_VIS].bytes = (size_t)geo_rays * ng * sizeof(double);    arr[O_VIS].produced = out->visibility != nullptr; own[O_VIS] = &ctx->b_vis;
    // in place (device pointers), into the device image of the caller's pinned window, or into buffers of the context: one rule
    // for the three products (cpol_place.h); the bases are added here
    PlacePlan plan;
    place_outputs(arr, A_N, p->outputs_on_device, ctx->keep_debug, &plan);
    const bool window = plan.window;
    void *T_all[A_N];
    if ((rc = place_resolve(ctx, arr, A_N, plan, own, T_all)) != CPOL_OK) return rc;
    void *const *const T = T_all, *const *const pr_T = T_all + A_PR;

    // the bucket counters start at zero: cleared by k_interp_sweep (no fill kernel); the domain
    // error word is sticky (cleared when reported)
    int *const d_errflag = ctx->d_errword;

    const bool tm = ctx->timing == 1;          // events around every stage
    const bool tm_psd = ctx->timing != 0;      // ... or only around the PSD stage
    if (tm_psd) {
        if (ctx->ev_used == ctx->ev_sets.size()) {
            hipEvent_t *set = new hipEvent_t[EV_N];
            for (int k = 0; k < EV_N; ++k) HIPCHK(hipEventCreate(&set[k]));
            ctx->ev_sets.push_back(set);
        }
        ctx->ev = ctx->ev_sets[ctx->ev_used++];
        if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_T0], st));
    }

    const auto ml_args = [&]() {            // k_ml_weights (on the values before melting), for the sweep and for the sub-beam export
        MlArgs ma{};
        ma.vals = (const float *)ctx->b_vals.p;
        ma.sub_w = (const double *)ctx->v_subw;
        ma.sub_smooth = (const int *)ctx->v_subsmooth;
        ma.taps = (const double *)ctx->v_mlfilter;
        ma.wgate = (double *)ctx->b_wgate.p;
        ma.n_sbg = n_sbg; ma.n_sub = n_sub; ma.n_gates = ng; ma.radius = t->ml_radius;
        ma.with_melting = p->with_melting;
        ma.var_qr = f.melt_qr; ma.var_qs = f.melt_qs; ma.var_qg = f.melt_qg;
        return ma;
    };

    // The launch sequence of a sweep.  Opt-in (CPOL_USE_GRAPH=1): with device outputs and
    // nothing to upload it is captured into a HIP graph and replayed while the arguments stay
    // the same (one graph launch instead of ten kernel launches).
    auto launch_all = [&]() -> int {
    // ---- 1. ray paths: evaluated inside k_interp_sweep; host-supplied paths are uploaded ----
    if (mode == CPOL_GEOM_HOST_PATHS) {
        HIPCHK(hipMemcpyAsync(ctx->b_traj.p, t->paths, (size_t)geo_rays * n_v * 3 * ng * sizeof(float),
                              hipMemcpyHostToDevice, st));
    }
    if (f.traj_launch) {
        // ray paths + per-ray constants ahead of the sweep kernel (and the parity access to the paths,
        // cpol_debug_read "traj"): same device functions as the in-place evaluation
        const bool paths = f.traj_paths;
        TrajArgs ta{};
        ta.ray_traj = (const double *)ctx->v_traj_in;
        ta.site = t->site ? (const double *)ctx->v_site : nullptr;
        ta.traj_out = paths ? (float *)ctx->b_traj.p : nullptr;
        ta.n_rays = geo_rays; ta.n_v = n_v; ta.n_gates = ng; ta.mode = mode;
        ta.range0 = p->range0; ta.range_step = p->range_step;
        ta.ke = p->ke; ta.re = p->re; ta.alt = p->radar_alt;
        ta.geo = (const double *)ctx->v_geo;
        ta.ray_const = f.ray_prep ? (double *)ctx->b_rayc.p : nullptr;
        ta.n_h = n_h; ta.lon1 = p->radar_lon;
        if (f.geo_poly) {
            ta.poly = (double *)ctx->b_poly.p;
            ta.poly_M = (const double *)ctx->d_geoM.p;
            ta.poly_scale = geo_poly_scale;
            ta.sin_u1 = p->sin_u1; ta.cos_u1 = p->cos_u1;
        }
        hipLaunchKernelGGL(k_trajectory, dim3((unsigned)(geo_rays * n_v), paths ? cdiv(ng, 256) : 1), dim3(256), 0, st, ctx->model, ta);
    }
    if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_TRAJ], st));

    // ---- 2. gate interpolation ----
    InterpArgs ia{};
    ia.traj = (mode == CPOL_GEOM_HOST_PATHS || f.prep_paths) ? (const float *)ctx->b_traj.p : nullptr;
    ia.ray_const = f.ray_prep ? (const double *)ctx->b_rayc.p : nullptr;
    ia.rp.ray_traj = (const double *)ctx->v_traj_in;
    ia.rp.site = t->site ? (const double *)ctx->v_site : nullptr;
    ia.rp.n_v = n_v; ia.rp.mode = mode;
    ia.rp.range0 = p->range0; ia.rp.range_step = p->range_step;
    ia.rp.ke = p->ke; ia.rp.re = p->re; ia.rp.alt = p->radar_alt;
    ia.zero_buf = cnt_next;
    ia.zero_n = (int)cnt_stride;
    ia.zero_buf2 = (int *)tot_next;     // (4 long long: k_classify / k_gate1 count the items outside the tables into them)
    ia.zero_n2 = 8;
    ia.geo = (const double *)ctx->v_geo;
    ia.sub_h = (const int *)ctx->v_subh;
    ia.sub_v = (const int *)ctx->v_subv;
    ia.vals = (float *)ctx->b_vals.p;
    ia.mask = (signed char *)ctx->b_mask.p;
    ia.elev = (float *)ctx->b_elev.p;
    ia.coords = ctx->keep_debug ? (float *)ctx->b_coords.p : nullptr;
    ia.lats = (double *)T[O_LAT];
    ia.lons = (double *)T[O_LON];
    ia.dist = (float *)T[O_DIST];
    ia.heights = (float *)T[O_HGT];
    ia.error_flag = d_errflag;
    ia.n_rays = geo_rays; ia.n_gates = ng; ia.n_sub = n_sub; ia.n_h = n_h; ia.n_v = n_v;
    ia.central_sub = n_sub / 2;
    ia.sin_u1 = p->sin_u1; ia.cos_u1 = p->cos_u1; ia.lon1 = p->radar_lon;
    ia.site = t->site ? (const double *)ctx->v_site : nullptr;
    ia.exact_sub = (p->debug_flags & CPOL_DEBUG_EXACT_SUBBEAMS) ? 1 : 0;
    // (the one sub-beam of a single-beam sweep: the polynomials of its table set, unless its float64 coordinates are outputs)
    if (f.drop_latlon) ia.lats = ia.lons = nullptr;
    ia.poly = f.geo_poly ? (const double *)ctx->b_poly.p : f.poly_single ? (const double *)set->poly.p : nullptr;
    ia.poly_scale = (f.geo_poly || f.poly_single) ? geo_poly_scale : 0.0;
    ia.poly_central = f.poly_single ? 1 : 0;
    if (f.present && CPOL_GATE1_PRESENT) {
        ia.present = (unsigned *)ctx->b_present.p;
        ia.n_pres = n_hyd;
        for (int j = 0; j < n_hyd; ++j) ia.pres_var[j] = ctx->hs.h[j].d.var_q;
    }
    ctx->last_poly_central = ia.poly_central;
    ctx->last_poly = ia.exact_sub ? nullptr : ia.poly;
    ctx->last_poly_fits = (long)geo_rays * n_h;
    if (cols) {
        // ---- 2'. the caller's columns instead of the interpolation ----
        const void *src[BUF_MAX_COLS];
        for (int k = 0; k < bp.n_col; ++k) {
            src[k] = col_src[k];
            if (!col_src[k] || cols->inputs_on_device) continue;
            void *d = (char *)ctx->b_colin.p + bp.col_off[k];
            HIPCHK(hipMemcpyAsync(d, col_src[k], bp.col_bytes[k], hipMemcpyHostToDevice, st));
            src[k] = d;
        }
        IngestArgs ig{};
        for (int v = 0; v < n_vars; ++v) ig.src_vals[v] = (const float *)src[v];
        ig.src_mask = (const signed char *)src[n_vars];
        ig.src_elev = (const float *)src[n_vars + 1];
        ig.src_wgate = (const double *)src[n_vars + 2];
        ig.src_q = (const float *)src[n_vars + 3];
        ig.src_fw = (const double *)src[n_vars + 4];
        ig.has_melting = (const signed char *)src[n_vars + 5];
        ig.vals = (float *)ctx->b_vals.p;
        ig.mask = (signed char *)ctx->b_mask.p;
        ig.elev = (float *)ctx->b_elev.p;
        ig.wgate = ml ? (double *)ctx->b_wgate.p : nullptr;
        ig.q_melt = (float *)ctx->b_qmelt.p;
        ig.fw_melt = (double *)ctx->b_fwmelt.p;
        ig.zero_buf = ia.zero_buf; ig.zero_n = ia.zero_n;
        ig.zero_buf2 = ia.zero_buf2; ig.zero_n2 = ia.zero_n2;
        ig.n_sbg = n_sbg; ig.n_vars = n_vars; ig.n_gates = ng;
        // (a grid-stride pass; at least enough workgroups to clear the counter set)
        const long blocks = std::max<long>(std::min<long>(cdiv(n_sbg, 256 * 4), 2048), cdiv(cnt_stride, 256));
        hipLaunchKernelGGL(k_columns_ingest, dim3((unsigned)blocks), dim3(256), 0, st, ig);
    } else if (mem) {
        // ---- 2m. the geometry of every sub-beam gate once, then the values of every member ----
        MemberArgs ma{};
        for (int k = 0; k < mem->n_members; ++k) ma.V[k] = mem->V[k];
        ma.n_members = mem->n_members;
        ma.n_sbg1 = (long)geo_rays * n_sub * ng;
        if (timed) {
            TimedArgs tg{};                 // (the per-ray brackets: uploaded above, with the work buffers)
            tg.ray_state = (const int *)ctx->b_timed.p;
            tg.ray_weight = (const float *)((const int32_t *)ctx->b_timed.p + n_rays);
            hipLaunchKernelGGL(k_interp_timed, dim3((unsigned)(geo_rays * n_sub), cdiv(ng, 256)), dim3(256), 0, st, ctx->model, ia, ma, tg);
        } else
        hipLaunchKernelGGL(k_interp_members, dim3((unsigned)(geo_rays * n_sub), cdiv(ng, 256)), dim3(256), 0, st, ctx->model, ia, ma);
    } else if (f.plain_interp) {
        // (the gate stencil of the (geometry, heights) pair where the rules allow it, cpol_forms.h: noted at first sight, recorded at
        // the second, replayed from the third on)
        int form = 0;
        StencilDev sd{};
        StencilEntry *made = nullptr;
        if (f.stencil) {
            StencilKey key;
            memset(&key, 0, sizeof key);
            key.version = t->version;
            key.heights = (ctx->parent ? ctx->parent : ctx)->st_heights;
            memcpy(key.shape, shape, sizeof shape);
            key.range0 = p->range0; key.range_step = p->range_step; key.ke = p->ke; key.re = p->re; key.alt = p->radar_alt;
            key.lon = p->radar_lon; key.sin_u1 = p->sin_u1; key.cos_u1 = p->cos_u1; key.poly_scale = ia.poly_scale;
            key.mode = mode; key.poly = (ia.poly ? 1 : 0) + 2 * ia.poly_central; key.exact = ia.exact_sub;
            form = stencil_pick(ctx, key, n_rg, &sd, &made);
        }
        const dim3 grid((unsigned)(n_rays * n_sub), cdiv(ng, 256));
        if (form == 2) {
            // (the replay with the cube's variable count as a constant -- one gather round for the 1-moment cubes, two of eight
            // variables for the 2-moment ones, each with and without EDR; every other count keeps the run-time loop)
            switch (CPOL_GATE1_PRESENT ? 0 : ctx->model.n_vars) {
            case 9: hipLaunchKernelGGL((k_interp_replay_n<9, 9>), grid, dim3(CPOL_REPLAY_THREADS), 0, st, ctx->model, ia, sd); break;
            case 10: hipLaunchKernelGGL((k_interp_replay_n<10, 10>), grid, dim3(CPOL_REPLAY_THREADS), 0, st, ctx->model, ia, sd); break;
            case 15: hipLaunchKernelGGL((k_interp_replay_n<15, 8>), grid, dim3(CPOL_REPLAY_THREADS), 0, st, ctx->model, ia, sd); break;
            case 16: hipLaunchKernelGGL((k_interp_replay_n<16, 8>), grid, dim3(CPOL_REPLAY_THREADS), 0, st, ctx->model, ia, sd); break;
            default: hipLaunchKernelGGL(k_interp_replay, grid, dim3(256), 0, st, ctx->model, ia, sd);
            }
        } else if (form == 1) {
            hipLaunchKernelGGL(k_interp_record, grid, dim3(256), 0, st, ctx->model, ia, sd);
            stencil_recorded(ctx, made);
        } else hipLaunchKernelGGL(k_interp_sweep, grid, dim3(256), 0, st, ctx->model, ia);
        ctx->last_stencil = form;
    }
    // ---- 2s. terrain shadowing: every sub-beam stays blocked behind its first gate below the topography (cpol_shadow.inl); the
    // forms that interpolate and go on in one launch are off (cpol_forms.h), so b_mask / b_vals hold the whole launch's columns ----
    if (shadow && !(pk.exp_skip & 1))
        hipLaunchKernelGGL(k_terrain_shadow, dim3((unsigned)cdiv((long)n_rays * n_sub, CPOL_SHADOW_THREADS / 64)), dim3(CPOL_SHADOW_THREADS), 0, st,
                           (signed char *)ctx->b_mask.p, (float *)ctx->b_vals.p, (long)n_rays * n_sub, ng, n_vars);
    // the visible share of the antenna pattern, from the codes as they now stand (the geometry rows: the first member's in an
    // ensemble call; the sum of the weights as FinalArgs::sum_w below).  The forms that interpolate inside the classifying kernel
    // write the codes there: the launch then follows that kernel
    const auto launch_visibility = [&]() {
        double sum_w = 0;
        for (int s = 0; s < n_sub; ++s) sum_w += t->sub_w[s];
        const long n_vis = (long)geo_rays * ng;
        hipLaunchKernelGGL(k_visibility, dim3((unsigned)cdiv(n_vis, 256)), dim3(256), 0, st, (const signed char *)ctx->b_mask.p,
                           (const double *)ctx->v_subw, (double *)T[O_VIS], n_vis, ng, n_sub, sum_w);
    };
    if (T[O_VIS] && !f.fused && !f.fused_gate1) launch_visibility();
    if (tm && !f.fused && !f.fused_gate1) HIPCHK(hipEventRecord(ctx->ev[EV_INTERP], st));
    if (sub_out) {
        // ---- 2''. cpol_interp_subbeams: geometry of every sub-beam, 'ml' weights, melting, copies; no scattering ----
        InterpArgs ix = ia;
        char *const xs = (char *)ctx->b_xscr.p, *const xg = (char *)ctx->b_xgeo.p;
        ix.vals = (float *)xs;
        ix.mask = (signed char *)(xs + bp.xscr_mask);
        ix.elev = (float *)(xs + bp.xscr_elev);
        ix.zero_buf = nullptr; ix.zero_buf2 = nullptr;
        ix.coords = nullptr; ix.lats = ix.lons = nullptr; ix.dist = ix.heights = nullptr;
        ix.present = nullptr;
        ix.exact_sub = 1;                         // (the long form: float64 latitude / longitude of every sub-beam)
        ExportArgs xa{};
        xa.lats = (double *)xg;
        xa.lons = (double *)(xg + bp.xgeo_lons);
        xa.dist = (float *)(xg + bp.xgeo_dist);
        xa.heights = (float *)(xg + bp.xgeo_heights);
        xa.elev = (float *)(xg + bp.xgeo_elev);
        signed char *const mlmask = (signed char *)(xg + bp.xgeo_mlmask);
        hipLaunchKernelGGL(k_interp_export, dim3((unsigned)(n_rays * n_sub), cdiv(ng, 256)), dim3(256), 0, st, ctx->model, ix, xa);
        if (ml) hipLaunchKernelGGL(k_ml_weights, dim3(n_rays * n_sub), dim3(64), 0, st, ml_args());
        if (f.sub_melt)
            hipLaunchKernelGGL(k_melt_subbeams, dim3((unsigned)cdiv(n_sbg, 256)), dim3(256), 0, st, (float *)ctx->b_vals.p, n_sbg,
                               f.melt_qr, f.melt_qs, f.melt_qg, (float *)ctx->b_qmelt.p, (double *)ctx->b_fwmelt.p, mlmask);
        const hipMemcpyKind kind = sub_out->outputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        struct Cp { void *dst; const void *src; size_t bytes; };
        const Cp cps[11] = {
            {sub_out->vals, ctx->b_vals.p, (size_t)n_vars * n_sbg * sizeof(float)},
            {sub_out->mask, ctx->b_mask.p, (size_t)n_sbg},
            {sub_out->elev, xa.elev, (size_t)n_sbg * sizeof(float)},
            {sub_out->lats, xa.lats, (size_t)n_sbg * sizeof(double)},
            {sub_out->lons, xa.lons, (size_t)n_sbg * sizeof(double)},
            {sub_out->dist, xa.dist, (size_t)n_sbg * sizeof(float)},
            {sub_out->heights, xa.heights, (size_t)n_sbg * sizeof(float)},
            {f.sub_melt ? sub_out->q_melt : nullptr, ctx->b_qmelt.p, (size_t)2 * n_sbg * sizeof(float)},
            {f.sub_melt ? sub_out->fw_melt : nullptr, ctx->b_fwmelt.p, (size_t)2 * n_sbg * sizeof(double)},
            {f.sub_melt ? sub_out->mask_ml : nullptr, mlmask, (size_t)n_sbg},
            {ml ? sub_out->wgate : nullptr, ctx->b_wgate.p, (size_t)n_sbg * sizeof(double)},
        };
        for (const Cp &c : cps)
            if (c.dst) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, kind, st));
        HIPCHK(hipGetLastError());
        return CPOL_OK;
    }

    // ---- 2b. the arguments of the final stage (k_gate1, the single-beam fast path, needs them already) ----
    FinalArgs fa{};
    fa.res = (const double *)ctx->b_res.p;
    fa.key = (const int *)ctx->b_key.p;
    fa.vmask = (const unsigned char *)ctx->b_vmask.p;
    fa.sub_mask = (const signed char *)ctx->b_mask.p;
    fa.vals = (const float *)ctx->b_vals.p;
    fa.sub_w = (const double *)ctx->v_subw;
    fa.sz_integ = bp.bytes[WB_SZINTEG] ? (float *)ctx->b_szinteg.p : nullptr;
    fa.sz_total = want_szt ? (float *)T[O_SZT] : nullptr;
    fa.ZH = (float *)T[O_ZH]; fa.ZV = (float *)T[O_ZV];
    fa.ZDR = (float *)T[O_ZDR]; fa.KDP = (float *)T[O_KDP];
    fa.DELTA_HV = (float *)T[O_DHV]; fa.RHOHV = (float *)T[O_RHOHV];
    fa.ATT_H = (float *)T[O_ATTH]; fa.ATT_V = (float *)T[O_ATTV];
    fa.mask = (double *)T[O_MASK];
    fa.mask8 = (signed char *)T[O_MASK8];
    fa.model_vars = want_model ? (double *)T[O_MODEL] : nullptr;
    fa.n_rays = n_rays; fa.n_gates = ng; fa.n_sub = n_sub; fa.n_hydro = n_hyd; fa.n_vars = n_vars;
    fa.c_zh = fa_c[0]; fa.c_kdp = fa_c[1]; fa.c_2w = fa_c[2];
    double sum_w = 0;
    for (int s = 0; s < n_sub; ++s) sum_w += t->sub_w[s];
    fa.sum_w = sum_w;
    fa.with_attenuation = p->with_attenuation;
    fa.res_km = (float)(p->radial_res / 1000.);
    fa.wgate = ml ? (const double *)ctx->b_wgate.p : nullptr;
    fa.RVEL = nullptr;
    if (doppler) {
        fa.RVEL = (double *)T[O_RVEL];
        fa.vn = (const double *)ctx->b_vn.p;
        fa.ice_first = (const IceFirst *)ctx->b_icefirst.p;
        fa.geo = (const double *)ctx->v_geo;
        fa.sub_h = (const int *)ctx->v_subh;
        fa.elev = (const float *)ctx->b_elev.p;
        fa.n_h = n_h;
        fa.var_u = p->var_u; fa.var_v = p->var_v; fa.var_w = p->var_w;
        fa.nyquist = t->nyquist ? (const double *)ctx->v_nyq : nullptr;
        for (int j = 0; j < n_hyd; ++j) fa.vsrc[j] = f.vsrc[j];
    }

    fa.eval_1d = f.final_inplace ? 1 : 0;
    fa.rec = (const double2 *)ctx->b_rec.p;
    for (int j = 0; j < n_hyd; ++j) fa.key_base[j] = ctx->hs.h[j].key_base;
    if (f.gate1) {
        fa.pre_gate = 1;
        fa.ice_redo = f.any_vsrc2 ? 1 : 0;
        fa.defer = (const unsigned char *)ctx->b_defer.p;
        fa.sk = (const float *)ctx->b_gscan.p;
        fa.sh = fa.sk + n_rg;
        fa.sv = fa.sk + 2 * n_rg;
    }

    // ---- 3. melting + PSD parameters + bucket histogram ----
    ClassifyArgs ca{};
    ca.vals = (float *)ctx->b_vals.p;
    ca.mask = (const signed char *)ctx->b_mask.p;
    ca.elev = (const float *)ctx->b_elev.p;
    ca.q_melt = ctx->keep_debug ? (float *)ctx->b_qmelt.p : nullptr;
    ca.fw_melt = ctx->keep_debug ? (double *)ctx->b_fwmelt.p : nullptr;
    ca.key = (int *)ctx->b_key.p;
    ca.pos = (int *)ctx->b_pos.p;
    ca.par = (double *)ctx->b_par.p;
    ca.count = cnt_p;
    ca.n_sbg = n_sbg;
    ca.present = ia.present;              // (k_gate1_ray: the presence words k_interp_sweep has just written)
    ca.with_melting = p->with_melting;
    ca.var_qr = f.melt_qr; ca.var_qs = f.melt_qs; ca.var_qg = f.melt_qg;
    ca.doppler = doppler ? 1 : 0;
    ca.tfun_snow = ctx->tfun[CPOL_TFUN_SNOW_N0];
    ca.tfun_ice = ctx->tfun[CPOL_TFUN_ICE_MOM2_A];
    // integral tables: not with Doppler scheme 3 + ice (k_spec_gate needs every item's parameters as
    // the integrating kernels leave them; the lookup writes the same slots, so it is fine) -- always on
    ca.n_lookup = cnt_p + n_keys + 1;
    ca.blk_ranked = (int *)ctx->b_blkranked.p;
    ca.rec = (double2 *)ctx->b_rec.p;
    ca.vmask = (unsigned char *)ctx->b_vmask.p;
    ca.vn = (doppler && !dop2 && !dop3) ? (double *)ctx->b_vn.p : nullptr;     // analytic moments (Doppler scheme 1)
    ca.keep_par = (ctx->keep_debug || dop3) ? 1 : 0;
    if (f.rare_direct) {
        ca.rare_key = (int *)ctx->b_pos.p;
        ca.rare_perm = (int *)ctx->b_perm.p;
        ca.rare_totals = (unsigned long long *)tot_p;
    }
    if (ml) {
        if (!cols) hipLaunchKernelGGL(k_ml_weights, dim3(n_rays * n_sub), dim3(64), 0, st, ml_args());     // (columns: ingested)
        ca.wgate = (const double *)ctx->b_wgate.p;
    }
    // the variables later kernels read: U, V, W (the Doppler terms); all of them for the integrated model variables
    ia.store_mask = want_model ? 0xffffffffu : 0u;
    if (doppler) ia.store_mask |= (1u << p->var_u) | (1u << p->var_v) | (1u << p->var_w);
    if (f.fused) {
        hipLaunchKernelGGL(k_interp_classify, dim3((unsigned)(n_rays * n_sub), cdiv(ng, 256)), dim3(256),
                           (size_t)n_vars * 256 * sizeof(float), st, ctx->model, ia, ctx->hs, ctx->its, ca);
        if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_INTERP], st));
    } else if (f.gate1) {
        GateArgs ga{};
        ga.sk = (float *)ctx->b_gscan.p;
        ga.sh = ga.sk + n_rg;
        ga.sv = ga.sk + 2 * n_rg;
        ga.defer = (unsigned char *)ctx->b_defer.p;
        ga.unit_key = (int *)ctx->b_pos.p;
        ga.perm = (int *)ctx->b_perm.p;
        ga.totals = (unsigned long long *)tot_p;
        ga.res = (double *)ctx->b_res.p;
        ga.store_items = f.any_vsrc2 ? 1 : 0;
        ga.analytic_vn = ca.vn ? 1 : 0;
        if (doppler) ca.vn = (double *)ctx->b_vn.p;        // (also the table-borne sums of a species summed over the ray)
        const bool melt_tab = f.any_2d, fused_gate1 = f.fused_gate1;
        const dim3 ggrid((unsigned)n_rays, cdiv(ng, CPOL_GATE1_THREADS));
        const size_t glds = (size_t)n_vars * CPOL_GATE1_THREADS * sizeof(float);
        if (f.gate1_ray) {
            // the whole rest of the sweep in this launch: no integrating kernels, no k_final
            ga.ticket = (int *)ctx->b_ticket.p;
            ScanRayArgs rr{};
            rr.PHIDP = (float *)T[O_PHIDP];
            rr.RVEL = nullptr;
            rr.sens_thr = cut ? (const double *)ctx->v_sens : nullptr;
            rr.radial_res = (float)p->radial_res;
            const size_t lds_terms = (size_t)n_hyd * (64 * GATE1S_BYTES + GATE1S_BLK_BYTES), lds_scan = (size_t)3 * ng * sizeof(float);
            const dim3 rgrid((unsigned)cdiv(ng, 64), (unsigned)n_rays);
            const dim3 tgrid((unsigned)gate1_tiles(n_rays, ng).n_blocks);      // k_gate1_ray: ray x gate tiles (cpol_tile.h)
            if (f.g1r == 3) {
                hipLaunchKernelGGL(k_gate1_ray_scan, rgrid, dim3(64 * n_hyd), lds_terms > lds_scan ? lds_terms : lds_scan, st,
                                   ctx->hs, ctx->its, ca, fa, ga, rr);
            } else {
                if (!(pk.exp_skip & 2))
                hipLaunchKernelGGL(k_gate1_ray, tgrid, dim3(64 * n_hyd), lds_terms, st, ctx->hs, ctx->its, ca, fa, ga, rr,
                                   gate1_finish_ops(fa, ga, t->sub_h, t->sub_w), gate1_species_set(ctx->hs, ctx->its, ca, fa, t->sub_w));
                if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_CLASSIFY], st));
                if (tm_psd) { HIPCHK(hipEventRecord(ctx->ev[EV_BUCKET], st)); HIPCHK(hipEventRecord(ctx->ev[EV_PSD], st)); }
                if (!(pk.exp_skip & 4))
                hipLaunchKernelGGL(k_scan_rays, dim3((unsigned)n_rays), dim3(256), lds_scan, st, fa, ga, rr);
                if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_FINAL], st));
                HIPCHK(hipGetLastError());
                return CPOL_OK;
            }
            if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_CLASSIFY], st));
            if (tm_psd) { HIPCHK(hipEventRecord(ctx->ev[EV_BUCKET], st)); HIPCHK(hipEventRecord(ctx->ev[EV_PSD], st)); }
            if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_FINAL], st));
            HIPCHK(hipGetLastError());
            return CPOL_OK;
        }
        if (f.by_species) hipLaunchKernelGGL(k_gate1_species, dim3((unsigned)cdiv(n_rg, 64)), dim3(64 * n_hyd),
                                           (size_t)n_hyd * (64 * GATE1S_BYTES + GATE1S_BLK_BYTES), st, ctx->hs, ctx->its, ca, fa, ga);
        else if (fused_gate1 && melt_tab) hipLaunchKernelGGL((k_interp_gate1<true>), ggrid, dim3(CPOL_GATE1_THREADS), glds, st,
                                                        ctx->model, ia, ctx->hs, ctx->its, ca, fa, ga);
        else if (fused_gate1) hipLaunchKernelGGL((k_interp_gate1<false>), ggrid, dim3(CPOL_GATE1_THREADS), glds, st,
                                                 ctx->model, ia, ctx->hs, ctx->its, ca, fa, ga);
        else if (melt_tab) hipLaunchKernelGGL((k_gate1<true>), dim3(cdiv(n_rg, CPOL_GATE1_THREADS)), dim3(CPOL_GATE1_THREADS), 0, st,
                                         ctx->hs, ctx->its, ca, fa, ga);
        else hipLaunchKernelGGL((k_gate1<false>), dim3(cdiv(n_rg, CPOL_GATE1_THREADS)), dim3(CPOL_GATE1_THREADS), 0, st,
                                ctx->hs, ctx->its, ca, fa, ga);
        if (tm && fused_gate1) HIPCHK(hipEventRecord(ctx->ev[EV_INTERP], st));
    } else if (melt_given) {
        ca.q_melt = (float *)ctx->b_qmelt.p;      // (inputs here: the caller's fields as k_columns_ingest left them)
        ca.fw_melt = (double *)ctx->b_fwmelt.p;
        hipLaunchKernelGGL(k_classify<true>, dim3(cdiv(n_sbg, CPOL_CLASSIFY_THREADS)),
                           dim3(CPOL_CLASSIFY_THREADS), 0, st, ctx->hs, ctx->its, ca);
    } else
    hipLaunchKernelGGL(k_classify<false>, dim3(cdiv(n_sbg, CPOL_CLASSIFY_THREADS)),
                       dim3(CPOL_CLASSIFY_THREADS), 0, st, ctx->hs, ctx->its, ca);
    if (T[O_VIS] && (f.fused || f.fused_gate1)) launch_visibility();
    if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_CLASSIFY], st));

    // ---- 4. counting sort by LUT slice ----
    ScanArgs sa{};
    sa.count = cnt_p;
    sa.offset = (int *)ctx->b_offset.p;
    sa.uoffset = (int *)ctx->b_offset.p + n_keys;
    sa.units = (WorkUnit *)ctx->b_units.p;
    sa.totals = tot_p;
    sa.n_keys = n_keys;
    sa.n_hydro = n_hyd;
    for (int j = 0; j < n_hyd; ++j) {
        const cpol_hydro_desc &d = ctx->hs.h[j].d;
        sa.key_base[j] = ctx->hs.h[j].key_base;
        sa.unit_shift[j] = ((d.psd_family == CPOL_PSD_GAMMA && d.uniform_grid) ||
                            (d.psd_family == CPOL_PSD_MELTING && d.tab_degree == CPOL_MELT_DEGREE) ||
                            (d.psd_family == CPOL_PSD_ICE_FIELD && d.uniform_grid && d.tab_degree == CPOL_ICE_DEGREE)) ? 7 : 6;
    }
    if (!f.rare_direct)
    hipLaunchKernelGGL(k_bucket_scan, dim3(1), dim3(1024), 0, st, sa);
    // (a fixed grid: the workgroups stride over the k_classify gate ranges and skip the empty ones)
    const long n_cblk = cdiv(n_sbg, CPOL_CLASSIFY_THREADS);
    if (!f.rare_direct)
    hipLaunchKernelGGL(k_bucket_scatter, dim3((unsigned)(n_cblk < 2048 ? n_cblk : 2048)), dim3(256), 0, st,
                       (const int *)ctx->b_key.p, (const int *)ctx->b_pos.p,
                       (int *)ctx->b_perm.p, (const int *)ctx->b_blkranked.p,
                       (const unsigned char *)ctx->b_vmask.p, n_sbg, n_hyd, sa);      // + the work-unit list
    if (tm_psd) HIPCHK(hipEventRecord(ctx->ev[EV_BUCKET], st));

    // ---- 5a. items on an integral table: 15 x 11 coefficients gathered, no diameter-bin loop ----
    if (f.any_tab) {
        LookupArgs la{};
        la.key = (const int *)ctx->b_key.p;
        la.vmask = (const unsigned char *)ctx->b_vmask.p;
        la.rec = (const double2 *)ctx->b_rec.p;
        la.par = (const double *)ctx->b_par.p;
        la.par_w = dop3 ? (double *)ctx->b_par.p : nullptr;
        la.res = (double *)ctx->b_res.p;
        la.vn = doppler ? (double *)ctx->b_vn.p : nullptr;
        la.n_sbg = n_sbg;
        la.skip_res_1d = (f.subsum || f.final_inplace) ? 1 : 0;
        la.vn_1d = f.final_inplace ? 1 : 0;
        la.tile = f.lookup_tile ? 1 : 0;
        la.n_rays = n_rays; la.n_sub = n_sub; la.n_gates = ng;
        la.split = f.lookup_split;
        long grid_x = cdiv(la.tile ? f.n_tiles * 64 : n_sbg, CPOL_LOOKUP_THREADS);
        if (f.use_tile_list && la.tile) {
            // a fixed grid walks the list: workgroups that own many tiles each: the chip filled `fill` times over (5 wavefronts per SIMD
            // resident), a workgroup's list never longer than its LDS array
            la.tile_scan = 1;
            la.n_tiles = f.n_tiles;
            for (int j = 0; j < n_hyd; ++j) if (ctx->its.t[j].tab && ctx->its.t[j].two_d) la.species2d |= 1u << j;
            const long cap_wg = std::max<long>(pk.lookup_fill * 1024 * 5 * CPOL_WAVE / CPOL_LOOKUP_THREADS, cdiv(f.n_tiles, CPOL_LOOKUP_LIST_CAP));
            if (grid_x > cap_wg) grid_x = cap_wg;
        }
        if (f.lookup_launch) {
            if (f.rare_fork) {             // k_psd_rare, below, goes to a sibling stream that forks HERE and joins before the sub-beam sums
                if (!ctx->ev_fork) HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
                HIPCHK(hipEventRecord(ctx->ev_fork, st));
            }
            hipLaunchKernelGGL(k_psd_lookup, dim3((unsigned)grid_x, la.split), dim3(CPOL_LOOKUP_THREADS), 0, st, ctx->hs, ctx->its, la);
        }
    }

    // ---- 5. PSD x scattering table: one launch per kernel flavour present ----
    {
        PsdArgs pa{};
        pa.unit_key = f.rare_direct ? (const int *)ctx->b_pos.p : nullptr;
        pa.units = (const WorkUnit *)ctx->b_units.p;
        pa.totals = tot_p;
        pa.perm = (const int *)ctx->b_perm.p;
        pa.par = (const double *)ctx->b_par.p;
        pa.res = (double *)ctx->b_res.p;
        pa.vn = doppler ? (double *)ctx->b_vn.p : nullptr;
        pa.n_sbg = n_sbg;
        pa.par_w = dop3 ? (double *)ctx->b_par.p : nullptr;
        pa.clk = nullptr;
        pa.ice_force_sum = pk.ice_force_sum;
        if (ctx->keep_debug) {
            HIPCHK(hipMemsetAsync(ctx->b_clk.p, 0, bp.bytes[WB_CLK], st));
            pa.clk = (long long *)ctx->b_clk.p;
        }
        // (items listed directly: the units are single items outside the tables, a handful per volume -- a small
        // grid costs an idle launch less; a flood of them is still processed, by 128 workgroups)
        const long cap_u = f.rare_direct ? 128 : pk.psd_grid, cap_g = f.rare_direct ? 128 : pk.psd_grid_generic;
        const dim3 grd_u((unsigned)(unit_cap < cap_u ? unit_cap : cap_u));
        const dim3 grd((unsigned)(unit_cap < cap_g ? unit_cap : cap_g)), blk(CPOL_PSD_THREADS);
        const int order[4] = {PSD_MODE_MELTING, PSD_MODE_ICE, PSD_MODE_GAMMA_UNIFORM, PSD_MODE_GAMMA_EXP};
        if (f.psd_rare_one) {              // ONE launch runs every flavour
            const int modes = f.psd_modes;
            pa.ice_same_launch = 1;
            hipStream_t sr = st;
            if (f.rare_fork) {
                if (!ctx->aux[0]) HIPCHK(hipStreamCreateWithFlags(&ctx->aux[0], hipStreamNonBlocking));
                if (!ctx->ev_join[0]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_join[0], hipEventDisableTiming));
                sr = ctx->aux[0];
                HIPCHK(hipStreamWaitEvent(sr, ctx->ev_fork, 0));
            }
            if (dop2) hipLaunchKernelGGL((k_psd_rare<true>), grd, blk, 0, sr, ctx->hs, pa, modes);
            else hipLaunchKernelGGL((k_psd_rare<false>), grd, blk, 0, sr, ctx->hs, pa, modes);
            if (f.rare_fork) {
                HIPCHK(hipEventRecord(ctx->ev_join[0], sr));
                HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[0], 0));
            }
        }
        const bool fork = f.psd_fork;
        if (fork) {
            if (!ctx->ev_fork) HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
            HIPCHK(hipEventRecord(ctx->ev_fork, st));
        }
        int n_aux = 0;
        for (int q = 0, launched = 0; q < 4; ++q) {
            const int M = order[q];
            if (!f.psd_need[M]) continue;
            hipStream_t s_ = st;
            if (fork && launched > 0) {
                const int i = n_aux++;
                if (!ctx->aux[i]) HIPCHK(hipStreamCreateWithFlags(&ctx->aux[i], hipStreamNonBlocking));
                if (!ctx->ev_join[i]) HIPCHK(hipEventCreateWithFlags(&ctx->ev_join[i], hipEventDisableTiming));
                s_ = ctx->aux[i];
                HIPCHK(hipStreamWaitEvent(s_, ctx->ev_fork, 0));
            }
            ++launched;
            switch (M) {
            case PSD_MODE_GAMMA_UNIFORM: {
                const dim3 blk_u(CPOL_PSD_THREADS_U);
                const size_t lds_pad = (size_t)pk.psd_lds_pad;
                if (dop2) hipLaunchKernelGGL((k_psd_uniform<true>), grd_u, blk_u, lds_pad, s_, ctx->hs, pa);
                else hipLaunchKernelGGL((k_psd_uniform<false>), grd_u, blk_u, lds_pad, s_, ctx->hs, pa);
                break; }
            case PSD_MODE_GAMMA_EXP:
                if (dop2) hipLaunchKernelGGL((k_psd<PSD_MODE_GAMMA_EXP, true>), grd, blk, 0, s_, ctx->hs, pa);
                else hipLaunchKernelGGL((k_psd<PSD_MODE_GAMMA_EXP, false>), grd, blk, 0, s_, ctx->hs, pa);
                break;
            case PSD_MODE_ICE:
                if (f.psd_ice_tab) {
                    if (dop2) hipLaunchKernelGGL((k_psd_ice2<true>), grd, blk, 0, s_, ctx->hs, pa);
                    else hipLaunchKernelGGL((k_psd_ice2<false>), grd, blk, 0, s_, ctx->hs, pa);
                }
                if (dop2) hipLaunchKernelGGL((k_psd<PSD_MODE_ICE, true>), grd, blk, 0, s_, ctx->hs, pa);
                else hipLaunchKernelGGL((k_psd<PSD_MODE_ICE, false>), grd, blk, 0, s_, ctx->hs, pa);
                break;
            default:
                if (f.psd_melt_tab) {
                    if (dop2) hipLaunchKernelGGL((k_psd_melting_tab<true>), grd, blk, 0, s_, ctx->hs, pa);
                    else hipLaunchKernelGGL((k_psd_melting_tab<false>), grd, blk, 0, s_, ctx->hs, pa);
                }
                if (f.psd_melt_direct) {
                    if (dop2) hipLaunchKernelGGL((k_psd_melting<true>), grd, blk, 0, s_, ctx->hs, pa);
                    else hipLaunchKernelGGL((k_psd_melting<false>), grd, blk, 0, s_, ctx->hs, pa);
                }
                break;
            }
            if (s_ != st) HIPCHK(hipEventRecord(ctx->ev_join[n_aux - 1], s_));
        }
        for (int i = 0; i < n_aux; ++i) HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[i], 0));
    }
    // ---- 5d. sub-beam sums per (gate, hydrometeor); the items on 1-D tables are evaluated here ----
    if (f.subsum) {
        SubsumArgs sa2{};
        sa2.key = (const int *)ctx->b_key.p;
        sa2.vmask = (const unsigned char *)ctx->b_vmask.p;
        sa2.rec = (const double2 *)ctx->b_rec.p;
        sa2.res = (const double *)ctx->b_res.p;
        sa2.vn = doppler ? (double *)ctx->b_vn.p : nullptr;
        sa2.sub_w = (const double *)ctx->v_subw;
        sa2.wgate = ml ? (const double *)ctx->b_wgate.p : nullptr;
        sa2.sz_integ = (float *)ctx->b_szinteg.p;
        sa2.n_rays = n_rays; sa2.n_gates = ng; sa2.n_sub = n_sub; sa2.n_hydro = n_hyd;
        const int tl = f.sum_tile_log2;   // lanes of a wavefront = a tile of neighbouring rays x consecutive gates
        sa2.tile_log2 = tl;
        sa2.coop_rounds = ctx->knobs.subsum_coop_rounds;
        const dim3 sgrid((unsigned)((long)cdiv(n_rays, CPOL_WAVE >> tl) * cdiv(ng, 1 << tl)), n_hyd);
#define CPOL_TEAM_CASE(W) case W: if (f.sum_chain) hipLaunchKernelGGL((k_subbeam_sum_team<W, true>), sgrid, dim3(CPOL_WAVE * W), 0, st, ctx->hs, ctx->its, sa2); \
                          else hipLaunchKernelGGL((k_subbeam_sum_team<W, false>), sgrid, dim3(CPOL_WAVE * W), 0, st, ctx->hs, ctx->its, sa2); break;
        switch (f.sum_form) {
        case SUM_TEAM:
            switch (f.sum_team) { CPOL_TEAM_CASE(2) CPOL_TEAM_CASE(3) CPOL_TEAM_CASE(4) CPOL_TEAM_CASE(5) CPOL_TEAM_CASE(6) CPOL_TEAM_CASE(7)
                                  case 8: hipLaunchKernelGGL((k_subbeam_sum_team<8, true>), sgrid, dim3(CPOL_WAVE * 8), 0, st, ctx->hs, ctx->its, sa2); break; }
            break;
#undef CPOL_TEAM_CASE
        case SUM_SCALAR: hipLaunchKernelGGL(k_subbeam_sum_scalar, sgrid, dim3(CPOL_SUBSUM_THREADS), 0, st, ctx->hs, ctx->its, sa2); break;
        case SUM_LDS: hipLaunchKernelGGL(k_subbeam_sum_lds, sgrid, dim3(CPOL_SUBSUM_THREADS), 0, st, ctx->hs, ctx->its, sa2); break;
        case SUM_SMALL: hipLaunchKernelGGL((k_subbeam_sum_gather<3, 10>), dim3(sgrid.x, n_hyd * 3), dim3(CPOL_SUBSUM_THREADS), 0, st, ctx->hs, ctx->its, sa2); break;
        default: hipLaunchKernelGGL((k_subbeam_sum_gather<1, 2>), sgrid, dim3(CPOL_SUBSUM_THREADS), 0, st, ctx->hs, ctx->its, sa2);
        }
    }
    if (tm_psd) HIPCHK(hipEventRecord(ctx->ev[EV_PSD], st));

    // ---- 6. accumulation + polarimetric variables + scans (the arguments: see 2b above) ----
    if (doppler)
        for (int j = 0; j < n_hyd && !dop3; ++j)
            if (f.vsrc[j] == 2)
                hipLaunchKernelGGL(k_ice_first, dim3(n_rays * n_sub), dim3(64), 0, st,
                                   (const unsigned char *)ctx->b_vmask.p, j,
                                   (const double *)ctx->b_vn.p + (long)j * n_sbg * 2,
                                   (IceFirst *)ctx->b_icefirst.p, ng);
    ScanRayArgs ra{};
    ra.PHIDP = (float *)T[O_PHIDP];
    ra.RVEL = nullptr;
    ra.sens_thr = cut ? (const double *)ctx->v_sens : nullptr;
    ra.radial_res = (float)p->radial_res;
    if (dop3) {
        // ---- 6b. Doppler spectrum (scheme 3): RVEL comes from the spectrum ----
        fa.RVEL = nullptr;
        SpecArgs sp{};
        sp.vals = (const float *)ctx->b_vals.p;
        sp.mask = (const signed char *)ctx->b_mask.p;
        sp.elev = (const float *)ctx->b_elev.p;
        sp.key = (const int *)ctx->b_key.p;
        sp.par = (const double *)ctx->b_par.p;
        sp.wgate = ml ? (const double *)ctx->b_wgate.p : nullptr;
        sp.geo = (const double *)ctx->v_geo;
        sp.sub_h = (const int *)ctx->v_subh;
        sp.varray = (const double *)ctx->v_varray;
        sp.beam = (float *)ctx->b_beam.p;
        sp.n_sbg = n_sbg; sp.n_gates = ng; sp.n_sub = n_sub; sp.n_h = n_h; sp.n_v = n_vb;
        sp.var_u = p->var_u; sp.var_v = p->var_v; sp.var_w = p->var_w; sp.var_rho = p->var_rho;
        sp.c_spec = (float)p->c_spectrum;
        sp.n_melt_rows = spec_melt ? 2 : 0;
        hipLaunchKernelGGL(k_spec_gate, dim3((unsigned)n_sbg), dim3(CPOL_SPEC_THREADS), spec_lds, st, ctx->hs, ctx->ss, sp);
        if (broaden) {
            // ---- turbulence / antenna motion: width and switch per sub-beam, then the filter row by row ----
            SpecWidthArgs wa{};
            wa.vals = (const float *)ctx->b_vals.p;
            wa.elev = (const float *)ctx->b_elev.p;
            wa.sigma = (double *)ctx->b_bsigma.p;
            wa.on = (int *)ctx->b_bon.p;
            wa.n_sbg = n_sbg; wa.n_gates = ng;
            wa.turb = p->turbulence_correction != 0; wa.motion = p->motion_correction != 0; wa.var_edr = p->var_edr;
            wa.range0 = p->range0; wa.range_step = p->range_step;
            wa.sigma_r = p->sigma_r; wa.sigma_theta = p->sigma_theta;
            wa.c_near = pow(CPOL_TURB_A, 3 / 2.); wa.c_far = pow(1.35 * CPOL_TURB_A, 3 / 2.);
            wa.motion_num = p->motion_num; wa.motion_den = p->motion_den;
            wa.v_res = p->v_res;
            hipLaunchKernelGGL(k_spec_width, dim3(n_rays * n_sub), dim3(64), 0, st, wa);
            SpecBroadenArgs ba{};
            ba.in = (const float *)ctx->b_beam.p; ba.out = (float *)ctx->b_beam.p;
            ba.sigma = (const double *)ctx->b_bsigma.p; ba.on = (const int *)ctx->b_bon.p;
            ba.rows_per_switch = ng; ba.n_v = n_vb;
            launch_broaden(ba, n_sbg, st);
        }
        if (p->with_attenuation) {
            SpecAttenArgs sa2{};
            sa2.key = (const int *)ctx->b_key.p;
            sa2.res = (const double *)ctx->b_res.p;
            sa2.beam = (float *)ctx->b_beam.p;
            sa2.n_sbg = n_sbg; sa2.n_gates = ng; sa2.n_v = n_vb; sa2.n_hydro = n_hyd;
            sa2.c_att = 4.343e-3 * 2 * p->wavelength;
            sa2.res_km = p->radial_res / 1000.;
            hipLaunchKernelGGL(k_spec_atten, dim3(n_rays * n_sub), dim3(64), (size_t)ng * sizeof(double), st, sa2);
        }
        SpecFinalArgs sf{};
        sf.beam = (const float *)ctx->b_beam.p;
        sf.sub_w = (const double *)ctx->v_subw;
        sf.wgate = ml ? (const double *)ctx->b_wgate.p : nullptr;
        sf.varray = (const double *)ctx->v_varray;
        sf.nyquist = t->nyquist ? (const double *)ctx->v_nyq : nullptr;
        sf.spectrum = (double *)T[O_SPEC];
        sf.RVEL = (double *)T[O_RVEL];
        sf.n_rays = n_rays; sf.n_gates = ng; sf.n_sub = n_sub; sf.n_v = n_vb;
        // cut_at_sensitivity censors the spectrum bin by bin (doppler_scatter.py:839-850)
        sf.sens_thr = cut ? (const double *)ctx->v_sens : nullptr;
        hipLaunchKernelGGL(k_spec_final, dim3((unsigned)n_rg), dim3(64), 0, st, sf);
        ra.RVEL = (double *)T[O_RVEL];       // censored with the other observables in k_final
    }
    fa.pre_integ = f.subsum ? 1 : 0;
    if (f.subsum) fa.sz_integ = (float *)ctx->b_szinteg.p;
    fa.proj = nullptr;
    if (f.rvel_terms) {
        // the per-sub-beam velocity terms by one thread per sub-beam gate (k_final adds them in order)
        hipLaunchKernelGGL(k_rvel_terms, dim3((unsigned)(n_rays * n_sub), cdiv(ng, 256)), dim3(256), 0, st,
                           fa, (double *)ctx->b_proj.p);
        fa.proj = (const double *)ctx->b_proj.p;
    }
    if (f.final_512)             // (one workgroup per ray; few rays: 512 threads halve its gate loop)
        hipLaunchKernelGGL((k_final<2 * CPOL_FINAL_THREADS>), dim3(n_rays), dim3(2 * CPOL_FINAL_THREADS), (size_t)3 * ng * sizeof(float), st, fa, ra, ctx->its);
    else
        hipLaunchKernelGGL((k_final<CPOL_FINAL_THREADS>), dim3(n_rays), dim3(CPOL_FINAL_THREADS), (size_t)3 * ng * sizeof(float), st, fa, ra, ctx->its);
    if (tm) HIPCHK(hipEventRecord(ctx->ev[EV_FINAL], st));
    HIPCHK(hipGetLastError());

    return CPOL_OK;
    };

    int forms[12];
    forms_record(fi, f, forms);
    memcpy(ctx->last_forms, forms, sizeof forms);
    ctx->last_stencil = 0;
    const double t_buffers = now_ns();
    ctx->counters_dirty = true;         // until the sequence is queued completely (cleared where sweep_serial advances)
    // graph key: every value that ends up in a kernel argument
    if (f.graphable) {
        uint64_t key = 1469598103934665603ull;
        auto mix = [&](const void *ptr, size_t n) {
            const unsigned char *c = (const unsigned char *)ptr;
            for (size_t i = 0; i < n; ++i) { key ^= c[i]; key *= 1099511628211ull; }
        };
        mix(p, sizeof *p);
        mix(&t->version, sizeof t->version);
        mix(T, O_N * sizeof *T);
        mix(&ctx->stage_serial, sizeof ctx->stage_serial);
        // (every work buffer the call sized, the per-ray tables, the stream, the table set's polynomials)
        int keyed[WB_N];
        const int n_keyed = buf_key_list(bp, keyed);
        for (int q = 0; q < n_keyed; ++q) mix(&(ctx->*WORK_BUFS[keyed[q]]).p, sizeof(void *));
        for (void **v : views) mix(v, sizeof *v);
        void *const more[] = {(void *)st, f.poly_single ? set->poly.p : nullptr};
        mix(more, sizeof more);
        // (the launch forms chosen above from state outside *p: a graph captured before the lanes were forked must not keep
        // replaying the four-launch sequence once k_gate1_ray is the default, nor the reverse)
        mix(forms, sizeof forms);
        hipGraphExec_t &gexec = ctx->graph_exec[par];
        if (!gexec || ctx->graph_key[par] != key) {
            if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; }
            hipGraph_t graph = nullptr;
            HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            const int lrc = launch_all();
            const hipError_t ce = hipStreamEndCapture(st, &graph);
            if (lrc != CPOL_OK || ce != hipSuccess || !graph) {
                if (graph) (void)hipGraphDestroy(graph);
                if (lrc != CPOL_OK) return lrc;
                ctx->err = "cpol_run_sweep: stream capture failed";
                return CPOL_ERR_HIP;
            }
            const hipError_t ie = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) { gexec = nullptr; ctx->err = "cpol_run_sweep: hipGraphInstantiate failed"; return CPOL_ERR_HIP; }
            ctx->graph_key[par] = key;
            ctx->graph_captures += 1;
        }
        HIPCHK(hipGraphLaunch(gexec, st));
        ctx->last_forms[11] = 1;
    } else {
        if ((rc = launch_all()) != CPOL_OK) return rc;
    }

    const double t_launched = now_ns();
    if (ctx->fail_next) {
        ctx->fail_next = false;
        ctx->err = "cpol_run_sweep: failure requested by the test hook (fail_next_sweep)";
        return CPOL_ERR_HIP;
    }
    // ---- the call's product behind the sequence (outside launch_all: the captured graph does not know it), on the per-gate fields
    // wherever they were placed (slot RVEL float64), into pr_T, where the plan placed the product's arrays ----
    const void *const fields[10] = {T[O_ZH], T[O_ZV], T[O_ZDR], T[O_KDP], T[O_DHV], T[O_PHIDP], T[O_RHOHV], T[O_ATTH], T[O_ATTV], T[O_RVEL]};
    switch (cq.product) {
    case PRODUCT_SUPEROB: rc = superob_launch(ctx, so, so_pl, fields, pr_T, ng, window, st); break;       // ONE kernel
    // the call's member(s) folded into the context's running state, and the outputs of a finishing call
    case PRODUCT_MEMBER_STATS: rc = member_stats_launch(ctx, ms, ms_pl, fields, pr_T, window, st, mv, p->outputs_on_device == 0); break;
    case PRODUCT_SPECTRUM_MOMENTS:                                                                        // ONE kernel, on the spectrum
        rc = spec_moments_launch(ctx, sm, (const double *)T[O_SPEC], (const double *)ctx->v_varray, pr_T, n_rg, n_vb, window, st);
        break;
    case PRODUCT_HISTOGRAM: {      // one kernel per requested field, into the context's running state; a finishing call's counts go to pr_T
        const int ord = hg->ordinate;
        const void *y = nullptr;
        long y_gates = n_rg;
        if (ord == HIST_ORD_HEIGHTS || ord == HIST_ORD_DIST) { y = T[ord == HIST_ORD_HEIGHTS ? O_HGT : O_DIST]; y_gates = (long)geo_rays * ng; }
        else if (ord >= HIST_ORD_MODEL) y = (const double *)T[O_MODEL] + (size_t)(ord - HIST_ORD_MODEL) * n_rg;
        else if (ord >= HIST_ORD_FIELD) y = fields[ord - HIST_ORD_FIELD];
        rc = hist_launch(ctx, hg, hg_pl, fields, y, y_gates, n_rg, ng, pr_T, st);
        break;
    }
    case PRODUCT_COMPOSITE:        // likewise; a finishing call decodes the state into the maps at pr_T
        rc = comp_launch(ctx, cp, cp_pl, fields, T[O_DIST], T[O_HGT], geo_rays, n_rg, ng, pr_T, 0, p->outputs_on_device != 1, st);
        // the neighbourhood verification: three kernels behind k_comp_finish, on the finished plane where the plan placed it
        if (rc == CPOL_OK && fr)
            rc = frac_launch(ctx, fr, fr_pl, ob_pl, (const float *)pr_T[fr_pl.field] + fr_pl.plane_first, fr_pl.plane_stride, p->outputs_on_device == 0,
                             pr_T + CP_N, st);
        break;
    case PRODUCT_SPECIES:          // ONE kernel, on the per-species rows and the delivered ZH: behind the range scans and the cut
        rc = species_launch(ctx, (const float *)ctx->b_szinteg.p, (const float *)T[O_ZH], pr_T, n_rg, n_hyd, fa_c[0], fa_c[1], fa_c[2], st);
        break;
    }
    if (rc != CPOL_OK) return rc;
    // ---- outputs that the kernels did not write in place ----
    if (window)
        HIPCHK(hipMemcpyAsync((void *)plan.win_lo, (const char *)ctx->b_outwin.p + plan.win_skew, (size_t)(plan.win_hi - plan.win_lo), hipMemcpyDeviceToHost, st));
    if ((rc = place_copy_out(ctx, arr, plan, T_all, dev)) != CPOL_OK) return rc;

    {
        const double t_done = now_ns();
        ctx->host_ns[0] += 1.0;
        ctx->host_ns[1] += t_tables - t_enter;
        ctx->host_ns[2] += t_buffers - t_tables;
        ctx->host_ns[3] += t_launched - t_buffers;
        ctx->host_ns[4] += t_done - t_launched;
        ctx->host_ns[5] += t_done - t_enter;
    }
    ctx->last_n_sbg = n_sbg; ctx->last_n_rg = n_rg; ctx->last_n_rays = n_rays;
    ctx->last_n_gates = ng; ctx->last_n_sub = n_sub; ctx->last_n_v = n_v;
    ctx->last_par = par;
    ++ctx->sweep_serial;
    ctx->counters_dirty = false;
    ctx->last_n_keys = n_keys; ctx->last_subsum = f.subsum || f.final_inplace;
    ctx->last_vmask = !f.gate1;
    ctx->last_vn = ctx->last_vmask && p->simulate_doppler == 1;
    ctx->last_icefirst = ctx->last_vn && f.any_vsrc2;
    ctx->counters.n_subbeam_gates = n_sbg;
    ctx->counters.n_gates = n_rg;

    if ((!dev && !async_host) || ctx->keep_debug) {
        // blocking host outputs: wait, then surface the domain error.  Device outputs and
        // non-blocking pinned-host outputs (outputs_on_device = 2) return at once: results
        // are valid, and a domain error is reported, after cpol_synchronize / cpol_counters.
        HIPCHK(hipStreamSynchronize(st));
        return report_domain_error(ctx);
    }
    return CPOL_OK;
}

int cpol_run_sweep(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_ray_tables_t *t,
                   cpol_outputs *out)
{
    return run_sequence(ctx, p, t, nullptr, nullptr, out);
}

int cpol_interp_subbeams(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_ray_tables_t *t, cpol_subbeam_outputs *so)
{
    if (!ctx) return CPOL_ERR_ARG;
    if (!p || !t || !so || so->outputs_on_device < 0 || so->outputs_on_device > 1) {
        ctx->err = "cpol_interp_subbeams: bad arguments (outputs_on_device is 0 or 1)";
        return CPOL_ERR_ARG;
    }
    cpol_sweep_params q = *p;
    q.outputs_on_device = so->outputs_on_device;
    q.apply_sensitivity = 0;
    q.integrate_model = 0;
    cpol_outputs none{};
    return run_sequence(ctx, &q, t, nullptr, so, &none);
}

int cpol_run_columns(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_columns_t *c, cpol_outputs *out)
{
    if (!ctx) return CPOL_ERR_ARG;
    const CallProduct cq = out ? call_product(CALL_COLUMNS, *out) : CallProduct{};      // (columns carry no product at all)
    if (cq.at_entry) { ctx->err = cq.refuse; return CPOL_ERR_ARG; }
    if (!p || !c || !out || p->n_rays < 1 || p->n_gates < 1 || p->n_sub < 1 || c->n_vars < 1 || c->n_vars > CPOL_MAX_VARS ||
        !c->vals || !c->elev || !c->sub_w) {
        ctx->err = "cpol_run_columns: bad shapes, or vals / elev / sub_w missing";
        return CPOL_ERR_ARG;
    }
    if ((long)p->n_rays * p->n_sub * p->n_gates >= (1L << 31)) {
        ctx->err = "cpol_run_columns: too many sub-beam gates in one call";
        return CPOL_ERR_ARG;
    }
    for (int v = 0; v < c->n_vars; ++v)
        if (!c->vals[v]) { ctx->err = "cpol_run_columns: a variable pointer of cols->vals is NULL"; return CPOL_ERR_ARG; }
    // every variable index of the staged descriptors must lie inside the caller's columns
    for (int j = 0; j < ctx->hs.n_hydro; ++j) {
        const cpol_hydro_desc &d = ctx->hs.h[j].d;
        if (d.var_t < 0 || d.var_t >= c->n_vars || (d.q_source == CPOL_Q_MODEL && (d.var_q < 0 || d.var_q >= c->n_vars)) ||
            (d.rule == CPOL_RULE_TWO_MOMENT && (d.var_qn < 0 || d.var_qn >= c->n_vars))) {
            ctx->err = "cpol_run_columns: a staged hydrometeor reads a variable beyond cols->n_vars";
            return CPOL_ERR_ARG;
        }
    }
    if (p->simulate_doppler && !c->az_sincos) { ctx->err = "cpol_run_columns: simulate_doppler needs cols->az_sincos"; return CPOL_ERR_ARG; }
    if (c->q_melt && (!c->fw_melt || !p->with_melting)) {
        ctx->err = "cpol_run_columns: cols->q_melt needs cols->fw_melt and with_melting";
        return CPOL_ERR_ARG;
    }
    // the per-ray tables of cpol_run_sweep for these columns: one horizontal and one vertical node per sub-beam, the
    // azimuth's sin / cos where the geo table has them (RVEL), no ray paths
    cpol_sweep_params q = *p;
    q.n_hnodes = q.n_vnodes = p->n_sub;
    q.geometry_mode = CPOL_GEOM_GROUND_43;
    std::vector<double> geo;
    std::vector<int32_t> ident;
    try {
        geo.assign((size_t)p->n_rays * p->n_sub * CPOL_GEO_STRIDE, 0.0);
        ident.resize((size_t)p->n_sub);
    } catch (...) {
        ctx->err = "cpol_run_columns: out of host memory";
        return CPOL_ERR_NOMEM;
    }
    if (c->az_sincos)
        for (size_t i = 0; i < (size_t)p->n_rays * p->n_sub; ++i) {
            geo[i * CPOL_GEO_STRIDE] = c->az_sincos[2 * i];
            geo[i * CPOL_GEO_STRIDE + 1] = c->az_sincos[2 * i + 1];
        }
    for (int s = 0; s < p->n_sub; ++s) ident[s] = s;
    cpol_ray_tables_t t{};
    t.geo = geo.data();
    t.sub_h = ident.data();
    t.sub_v = ident.data();
    t.sub_w = c->sub_w;
    t.sens_thr = c->sens_thr;
    t.nyquist = c->nyquist;
    t.varray = c->varray;
    return run_sequence(ctx, &q, &t, c, nullptr, out);
}

int cpol_run_sweep_members(cpol_ctx *ctx, const cpol_sweep_params *p, const cpol_ray_tables_t *t, const int32_t *members,
                           int n_members, cpol_outputs *out)
{
    if (!ctx) return CPOL_ERR_ARG;
    if (!p || !t || !out || !members || n_members < 1 || n_members > CPOL_MEMBERS_PER_CALL || p->n_rays < 1 || p->n_vnodes < 1 ||
        p->n_hnodes < 1 || !t->traj || !t->geo) {
        ctx->err = "cpol_run_sweep_members: bad arguments (1 <= n_members <= 64 per call)";
        return CPOL_ERR_ARG;
    }
    const CallProduct cq = call_product(CALL_MEMBERS, *out);                            // (members carry no spectrum moments)
    if (cq.at_entry) { ctx->err = cq.refuse; return CPOL_ERR_ARG; }
    if (t->time_blend != 0) {
        // ---- ONE scan, every ray blended from the two states that bracket its time ----
        if (t->time_blend != 1 || !t->ray_state || !t->ray_weight) {
            ctx->err = "cpol_run_sweep_members: time_blend is 0 or 1 and needs ray_state and ray_weight";
            return CPOL_ERR_ARG;
        }
        if (p->geometry_mode != CPOL_GEOM_GROUND_43) {
            ctx->err = "cpol_run_sweep_members: time_blend takes ground radars on the 4/3-earth ray paths (no spaceborne geometry, no host paths)";
            return CPOL_ERR_ARG;
        }
        MembersCall mc{};
        mc.n_members = n_members;
        mc.n_rays = p->n_rays;
        mc.timed = true;
        mc.ray_state = t->ray_state;
        mc.ray_weight = t->ray_weight;
        for (int k = 0; k < n_members; ++k) {
            mc.V[k] = member_cube(ctx, members[k]);
            if (!mc.V[k]) { ctx->err = "cpol_run_sweep_members: a requested member is not staged"; return CPOL_ERR_ARG; }
        }
        for (int r = 0; r < p->n_rays; ++r) {
            const int32_t lo = t->ray_state[r];
            const float w = t->ray_weight[r];
            if (!(w >= 0.0f && w < 1.0f)) {             // (NaN fails both)
                ctx->err = "cpol_run_sweep_members: time_blend: a ray_weight outside [0, 1) or not finite";
                return CPOL_ERR_ARG;
            }
            if (lo < 0 || lo >= n_members || (w != 0.0f && lo + 1 >= n_members)) {
                ctx->err = "cpol_run_sweep_members: time_blend: a ray_state (or the state behind it, with a weight > 0) outside `members`";
                return CPOL_ERR_ARG;
            }
        }
        return run_sequence(ctx, p, t, nullptr, nullptr, out, &mc);
    }
    if (out->model_vars) {
        ctx->err = "cpol_run_sweep_members: antenna-integrated model variables are not part of an ensemble call (outputs->model_vars must be NULL)";
        return CPOL_ERR_ARG;
    }
    MembersCall mc{};
    mc.n_members = n_members;
    mc.n_rays = p->n_rays;
    for (int k = 0; k < n_members; ++k) {
        mc.V[k] = member_cube(ctx, members[k]);
        if (!mc.V[k]) { ctx->err = "cpol_run_sweep_members: a requested member is not staged"; return CPOL_ERR_ARG; }
        for (int j = 0; j < k; ++j)
            if (members[j] == members[k]) { ctx->err = "cpol_run_sweep_members: a member is requested twice"; return CPOL_ERR_ARG; }
    }
    if ((long)p->n_rays * n_members >= (1L << 31)) { ctx->err = "cpol_run_sweep_members: too many rows"; return CPOL_ERR_ARG; }
    // the second half runs over n_members * n_rays rows, row m * n_rays + r = ray r of member m: the per-ray tables repeated
    const size_t nr = (size_t)p->n_rays, M = (size_t)n_members;
    const size_t w_traj = (size_t)p->n_vnodes * CPOL_TRAJ_STRIDE, w_geo = (size_t)p->n_hnodes * CPOL_GEO_STRIDE;
    std::vector<double> traj, geo, site, nyq;
    try {
        traj.resize(M * nr * w_traj);
        geo.resize(M * nr * w_geo);
        if (t->site) site.resize(M * nr * CPOL_SITE_STRIDE);
        if (t->nyquist) nyq.resize(M * nr);
    } catch (...) {
        ctx->err = "cpol_run_sweep_members: out of host memory";
        return CPOL_ERR_NOMEM;
    }
    for (size_t k = 0; k < M; ++k) {
        memcpy(traj.data() + k * nr * w_traj, t->traj, nr * w_traj * sizeof(double));
        memcpy(geo.data() + k * nr * w_geo, t->geo, nr * w_geo * sizeof(double));
        if (t->site) memcpy(site.data() + k * nr * CPOL_SITE_STRIDE, t->site, nr * CPOL_SITE_STRIDE * sizeof(double));
        if (t->nyquist) memcpy(nyq.data() + k * nr, t->nyquist, nr * sizeof(double));
    }
    cpol_ray_tables_t tt = *t;
    tt.traj = traj.data();
    tt.geo = geo.data();
    if (t->site) tt.site = site.data();
    if (t->nyquist) tt.nyquist = nyq.data();
    cpol_sweep_params q = *p;
    q.n_rays = p->n_rays * n_members;
    q.integrate_model = 0;
    return run_sequence(ctx, &q, &tt, nullptr, nullptr, out, &mc);
}

int cpol_spaceborne_first_gate(cpol_ctx *ctx, const cpol_sweep_params *p, const double *traj,
                               const double *site, const int32_t *n_cand, double ceiling_m,
                               int32_t *first_gate)
{
    if (!ctx || !p || !traj || !site || !n_cand || !first_gate || p->n_rays < 1 || p->n_vnodes < 1) {
        if (ctx) ctx->err = "cpol_spaceborne_first_gate: bad arguments";
        return CPOL_ERR_ARG;
    }
    (void)hipGetLastError();            // a stale error of another user of the runtime in this thread is not ours
    HIPCHK(hipSetDevice(ctx->device));
    const int n = p->n_rays * p->n_vnodes;
    DevBuf d_tr, d_site, d_nc, d_out;
    int rc;
    if ((rc = upload(ctx, d_tr, traj, (size_t)n * 4 * sizeof(double)))) return rc;
    if ((rc = upload(ctx, d_site, site, (size_t)p->n_rays * 8 * sizeof(double)))) return rc;
    if ((rc = upload(ctx, d_nc, n_cand, (size_t)p->n_rays * sizeof(int)))) return rc;
    if ((rc = ensure(ctx, d_out, (size_t)n * sizeof(int)))) return rc;
    hipLaunchKernelGGL(k_spaceborne_first_gate, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream,
                       (const double *)d_tr.p, (const double *)d_site.p, (const int *)d_nc.p,
                       (int *)d_out.p, p->n_rays, p->n_vnodes, p->range0, p->range_step, ceiling_m);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(first_gate, d_out.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    free_buf(d_tr); free_buf(d_site); free_buf(d_nc); free_buf(d_out);
    return CPOL_OK;
}

int cpol_counters(cpol_ctx *ctx, cpol_counters_t *out)
{
    if (!ctx || !out) return CPOL_ERR_ARG;
    if (ctx->last_n_sbg > 0) {
        // device-side totals of the LAST sweep (valid once the stream drained)
        HIPCHK(hipStreamSynchronize(ctx->stream));
        long long totals[2] = {0, 0};
        HIPCHK(hipMemcpy(totals, (const long long *)ctx->b_totals.p + ctx->last_par * 4, sizeof totals, hipMemcpyDeviceToHost));
        long long n_lookup = 0;
        {
            std::vector<int> slots(CPOL_COUNT_SLOTS);       // the kernels count into one of many words (count_table_items)
            HIPCHK(hipMemcpy(slots.data(), (const int *)ctx->b_count.p + ctx->last_par * ctx->count_stride + ctx->last_n_keys + 3, slots.size() * sizeof(int), hipMemcpyDeviceToHost));
            for (int v : slots) n_lookup += v;
        }
        ctx->counters.n_table_items = n_lookup;
        totals[0] += n_lookup;                              // valid items = integrated + looked up
        ctx->counters.n_valid_items = totals[0];
        ctx->counters.n_work_units = totals[1];
        if (ctx->ev_used > 0) {
            // average stage durations over the sweeps recorded since enable_timing
            double acc[EV_N] = {}, tot = 0;
            for (size_t i = 0; i < ctx->ev_used; ++i) {
                hipEvent_t *e = ctx->ev_sets[i];
                float ms = 0;
                if (ctx->timing == 2) {                     // PSD stage only
                    HIPCHK(hipEventElapsedTime(&ms, e[EV_BUCKET], e[EV_PSD]));
                    acc[EV_PSD] += ms;
                    continue;
                }
                for (int k = 1; k < EV_N; ++k) {
                    HIPCHK(hipEventElapsedTime(&ms, e[k - 1], e[k]));
                    acc[k] += ms;
                }
                HIPCHK(hipEventElapsedTime(&ms, e[EV_T0], e[EV_FINAL]));
                tot += ms;
            }
            const double inv = 1.0 / (double)ctx->ev_used;
            ctx->counters.ms_traj = (float)(acc[EV_TRAJ] * inv);
            ctx->counters.ms_interp = (float)(acc[EV_INTERP] * inv);
            ctx->counters.ms_classify = (float)(acc[EV_CLASSIFY] * inv);
            ctx->counters.ms_bucket = (float)(acc[EV_BUCKET] * inv);
            ctx->counters.ms_psd = (float)(acc[EV_PSD] * inv);
            ctx->counters.ms_final = (float)(acc[EV_FINAL] * inv);
            ctx->counters.ms_total = (float)(tot * inv);
        }
        *out = ctx->counters;
        return report_domain_error(ctx);
    }
    *out = ctx->counters;
    return CPOL_OK;
}

int cpol_debug_scan(cpol_ctx *ctx, int form, int mul, const float *x, float *y, int n_rows, int n)
{
    if (!ctx) return CPOL_ERR_ARG;
    if (!x || !y || n_rows < 1 || n_rows > 65535 || n < 1 || (size_t)n * sizeof(float) > 64 * 1024 || form < 0 || form > 1) {
        ctx->err = "cpol_debug_scan: form 0 / 1, 1 <= n_rows <= 65535, 1 <= n <= 16384 (a row of float32 in 64 KB of LDS)";
        return CPOL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n_rows * n * sizeof(float), lds = (size_t)n * sizeof(float);
    DevBuf dx, dy;
    int rc;
    if ((rc = upload(ctx, dx, x, bytes))) return rc;
    if ((rc = ensure(ctx, dy, bytes))) { free_buf(dx); return rc; }
    const dim3 grid((unsigned)n_rows), block(64);
    const float *px = (const float *)dx.p;
    float *py = (float *)dy.p;
    if (form == 1 && mul) hipLaunchKernelGGL((k_debug_scan<true, true>), grid, block, lds, ctx->stream, px, py, n);
    else if (form == 1) hipLaunchKernelGGL((k_debug_scan<false, true>), grid, block, lds, ctx->stream, px, py, n);
    else if (mul) hipLaunchKernelGGL((k_debug_scan<true, false>), grid, block, lds, ctx->stream, px, py, n);
    else hipLaunchKernelGGL((k_debug_scan<false, false>), grid, block, lds, ctx->stream, px, py, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(y, dy.p, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    free_buf(dx);
    free_buf(dy);
    if (e != hipSuccess) { ctx->err = std::string("cpol_debug_scan: ") + hipGetErrorString(e); return CPOL_ERR_HIP; }
    return CPOL_OK;
}

// The test hook cpol_debug_read "terrain_shadow_rows": k_terrain_shadow alone on caller arrays (host memory, in and out, blocking) --
// rows no sweep produces (every position of the first hit against the 64-gate chunks, finite values under a hit)
struct ShadowHook {
    int32_t n_rows, n_gates, n_vars, pad_;
    int8_t *mask;                           // [n_rows][n_gates] codes, shadowed in place
    float *vals;                            // [n_vars][n_rows * n_gates], shadowed in place
};

static int shadow_hook(cpol_ctx *ctx, const ShadowHook *h)
{
    int8_t *const mask = h->mask;
    float *const vals = h->vals;
    const int n_rows = h->n_rows, n_gates = h->n_gates, n_vars = h->n_vars;
    if (!mask || !vals || n_rows < 1 || n_gates < 1 || n_vars < 1 || n_vars > CPOL_MAX_VARS || (long)n_rows * n_gates >= (1L << 31)) {
        ctx->err = "cpol_debug_read(terrain_shadow_rows): mask and vals, n_rows, n_gates >= 1, 1 <= n_vars <= CPOL_MAX_VARS, n_rows * n_gates < 2^31";
        return CPOL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t mb = (size_t)n_rows * n_gates, vb = mb * n_vars * sizeof(float);
    DevBuf dm, dv;
    int rc;
    if ((rc = upload(ctx, dm, mask, mb))) return rc;
    if ((rc = upload(ctx, dv, vals, vb))) { free_buf(dm); return rc; }
    hipLaunchKernelGGL(k_terrain_shadow, dim3((unsigned)cdiv((long)n_rows, CPOL_SHADOW_THREADS / 64)), dim3(CPOL_SHADOW_THREADS), 0, ctx->stream,
                       (signed char *)dm.p, (float *)dv.p, (long)n_rows, n_gates, n_vars);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(mask, dm.p, mb, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(vals, dv.p, vb, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    free_buf(dm);
    free_buf(dv);
    if (e != hipSuccess) { ctx->err = std::string("cpol_debug_read(terrain_shadow_rows): ") + hipGetErrorString(e); return CPOL_ERR_HIP; }
    return CPOL_OK;
}

int cpol_debug_math(cpol_ctx *ctx, int op, const double *x, double *y, int n)
{
    if (!ctx || !x || !y || n < 1) return CPOL_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf dx, dy;
    int rc;
    if ((rc = upload(ctx, dx, x, (size_t)n * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, dy, (size_t)n * sizeof(double)))) { free_buf(dx); return rc; }
    hipLaunchKernelGGL(k_debug_math, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, op,
                       (const double *)dx.p, (double *)dy.p, n);
    hipError_t e = hipMemcpyAsync(y, dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    free_buf(dx);
    free_buf(dy);
    if (e != hipSuccess) { ctx->err = std::string("cpol_debug_math: ") + hipGetErrorString(e); return CPOL_ERR_HIP; }
    return CPOL_OK;
}

int64_t cpol_debug_read(cpol_ctx *ctx, const char *name, void *dst, int64_t max_bytes)
{
    if (!ctx || !name) return CPOL_ERR_ARG;
    if (!strcmp(name, "enable")) { ctx->keep_debug = true; return 0; }
    if (!strcmp(name, "disable")) { ctx->keep_debug = false; return 0; }
    if (!strcmp(name, "fail_next_sweep")) { ctx->fail_next = true; return 0; }
    if (!strcmp(name, "poly_central")) {
        if (!dst || max_bytes < (int64_t)sizeof(int)) return CPOL_ERR_ARG;
        memcpy(dst, &ctx->last_poly_central, sizeof(int));
        return (int64_t)sizeof(int);
    }
    if (!strcmp(name, "stencil")) {
        // gate stencils: [the form of this context's last sweep (0 full, 1 recording, 2 replay), entries of the root's store, bytes it
        // holds, records made, replays, entries dropped]
        cpol_ctx *own = ctx->parent ? ctx->parent : ctx;
        std::lock_guard<std::mutex> lk(own->st_mu);
        const double v[6] = {(double)ctx->last_stencil, (double)own->st_entries.size(), (double)own->st_bytes, (double)own->st_records,
                             (double)own->st_replays, (double)own->st_drops};
        if (!dst || max_bytes < (int64_t)sizeof v) return CPOL_ERR_ARG;
        memcpy(dst, v, sizeof v);
        return (int64_t)sizeof v;
    }
    if (!strcmp(name, "member_stats_fields")) {     // a CONTROL name: dst points to a MemberStatsHook
        if (!dst || max_bytes < (int64_t)sizeof(MemberStatsHook)) { ctx->err = "cpol_debug_read(member_stats_fields): dst = the hook's struct"; return CPOL_ERR_ARG; }
        return member_stats_hook(ctx, (const MemberStatsHook *)dst);
    }
    if (!strcmp(name, "member_verify_fields")) {    // a CONTROL name: dst points to a MemberVerifyHook
        if (!dst || max_bytes < (int64_t)sizeof(MemberVerifyHook)) { ctx->err = "cpol_debug_read(member_verify_fields): dst = the hook's struct"; return CPOL_ERR_ARG; }
        return member_stats_hook(ctx, (const MemberStatsHook *)dst, &((const MemberVerifyHook *)dst)->mv);
    }
    if (!strcmp(name, "spectrum_moments_rows")) {   // a CONTROL name: dst points to a SpecMomentsHook
        if (!dst || max_bytes < (int64_t)sizeof(SpecMomentsHook)) { ctx->err = "cpol_debug_read(spectrum_moments_rows): dst = the hook's struct"; return CPOL_ERR_ARG; }
        return spec_moments_hook(ctx, (const SpecMomentsHook *)dst);
    }
    if (!strcmp(name, "histogram_fields")) {        // a CONTROL name: dst points to a HistHook
        if (!dst || max_bytes < (int64_t)sizeof(HistHook)) { ctx->err = "cpol_debug_read(histogram_fields): dst = the hook's struct"; return CPOL_ERR_ARG; }
        return hist_hook(ctx, (const HistHook *)dst);
    }
    if (!strcmp(name, "species_fields")) {          // a CONTROL name: dst points to a SpeciesHook
        if (!dst || max_bytes < (int64_t)sizeof(SpeciesHook)) { ctx->err = "cpol_debug_read(species_fields): dst = the hook's struct"; return CPOL_ERR_ARG; }
        return species_hook(ctx, (const SpeciesHook *)dst);
    }
    if (!strcmp(name, "histogram_stretch")) {
        if (!dst || max_bytes < (int64_t)sizeof(int32_t)) return CPOL_ERR_ARG;
        const int32_t v = HIST_STRETCH;
        memcpy(dst, &v, sizeof v);
        return (int64_t)sizeof v;
    }
    if (!strcmp(name, "composite_fields")) {        // a CONTROL name: dst points to a CompHook
        if (!dst || max_bytes < (int64_t)sizeof(CompHook)) { ctx->err = "cpol_debug_read(composite_fields): dst = the hook's struct"; return CPOL_ERR_ARG; }
        if ((((const CompHook *)dst)->c.products & CPOL_COMP_SUM) && max_bytes < (int64_t)(offsetof(CompHook, c) + sizeof(cpol_composite_sums))) {
            ctx->err = "cpol_debug_read(composite_fields): with CPOL_COMP_SUM the hook's struct ends in a cpol_composite_sums";
            return CPOL_ERR_ARG;
        }
        return comp_hook(ctx, (const CompHook *)dst);
    }
    if (!strcmp(name, "fractions_maps")) {          // a CONTROL name: dst points to a FracHook
        if (!dst || max_bytes < (int64_t)sizeof(FracHook)) { ctx->err = "cpol_debug_read(fractions_maps): dst = the hook's struct"; return CPOL_ERR_ARG; }
        if (frac_is_ensemble(&((const FracHook *)dst)->f) && max_bytes < (int64_t)(sizeof(FracHook) + sizeof(void *))) {
            ctx->err = "cpol_debug_read(fractions_maps): CPOL_FRAC_ENSEMBLE needs the pointer behind f";
            return CPOL_ERR_ARG;
        }
        return frac_hook(ctx, (const FracHook *)dst);
    }
    if (!strcmp(name, "composite_plane")) {         // {uploads, hits} of this context's gate-plane store
        if (!dst || max_bytes < (int64_t)sizeof ctx->cplane_stat) return CPOL_ERR_ARG;
        memcpy(dst, ctx->cplane_stat, sizeof ctx->cplane_stat);
        return (int64_t)sizeof ctx->cplane_stat;
    }
    if (!strcmp(name, "composite_stretch")) {
        if (!dst || max_bytes < (int64_t)sizeof(int32_t)) return CPOL_ERR_ARG;
        const int32_t v = COMP_STRETCH;
        memcpy(dst, &v, sizeof v);
        return (int64_t)sizeof v;
    }
    if (!strcmp(name, "terrain_shadow_rows")) {     // a CONTROL name: dst points to a ShadowHook
        if (!dst || max_bytes < (int64_t)sizeof(ShadowHook)) { ctx->err = "cpol_debug_read(terrain_shadow_rows): dst = the hook's struct"; return CPOL_ERR_ARG; }
        return shadow_hook(ctx, (const ShadowHook *)dst);
    }
    if (!strcmp(name, "superob_fields")) {          // a CONTROL name: dst points to a SuperobHook
        if (!dst || max_bytes < (int64_t)sizeof(SuperobHook)) { ctx->err = "cpol_debug_read(superob_fields): dst = the hook's struct"; return CPOL_ERR_ARG; }
        return superob_hook(ctx, (const SuperobHook *)dst);
    }
    if (!strcmp(name, "stencil_budget")) {
        // a CONTROL name like "enable": *dst = uint64 bytes the root's store may hold (0: stencils off; default 1 GiB).  Refused while
        // lanes exist; lowering it below what the store holds drops every entry (the root's stream is drained first)
        if (!dst || max_bytes < (int64_t)sizeof(uint64_t)) { ctx->err = "cpol_debug_read(stencil_budget): dst = uint64 bytes"; return CPOL_ERR_ARG; }
        if (model_on_lane(ctx, "cpol_debug_read(stencil_budget)")) return CPOL_ERR_ARG;
        uint64_t bytes;
        memcpy(&bytes, dst, sizeof bytes);
        bool drop;
        {
            std::lock_guard<std::mutex> lk(ctx->st_mu);
            drop = (size_t)bytes < ctx->st_bytes || bytes == 0;
            ctx->st_budget = (size_t)bytes;
            for (StencilEntry *e : ctx->st_entries) if (!e->buf) e->refused = false;
        }
        if (drop) { HIPCHK(hipSetDevice(ctx->device)); stencil_drop_all(ctx); }
        return 0;
    }
    if (!strcmp(name, "launch_forms")) {
        if (!dst || max_bytes < (int64_t)sizeof ctx->last_forms) return CPOL_ERR_ARG;
        memcpy(dst, ctx->last_forms, sizeof ctx->last_forms);
        return (int64_t)sizeof ctx->last_forms;
    }
    if (!strcmp(name, "graph_captures")) {
        if (!dst || max_bytes < (int64_t)sizeof ctx->graph_captures) return CPOL_ERR_ARG;
        memcpy(dst, &ctx->graph_captures, sizeof ctx->graph_captures);
        return (int64_t)sizeof ctx->graph_captures;
    }
    if (!strcmp(name, "work_buffers")) {
        // the capacity of every per-sweep work buffer in the order of enum WorkBuf (cpol_buffers.h), 0: absent; a test hook like "geo_poly"
        uint64_t cap[WB_N];
        if (!dst || max_bytes < (int64_t)sizeof cap) return CPOL_ERR_ARG;
        for (int w = 0; w < WB_N; ++w) { const DevBuf &b = ctx->*WORK_BUFS[w]; cap[w] = b.p ? b.cap : 0; }
        memcpy(dst, cap, sizeof cap);
        return (int64_t)sizeof cap;
    }
    if (!strcmp(name, "host_times")) {
        // host time of cpol_run_sweep by section since the last read (see cpol_ctx::host_ns); reading resets
        if (!dst || max_bytes < (int64_t)sizeof ctx->host_ns) return CPOL_ERR_ARG;
        memcpy(dst, ctx->host_ns, sizeof ctx->host_ns);
        for (double &v : ctx->host_ns) v = 0.0;
        return (int64_t)sizeof ctx->host_ns;
    }
    if (!strcmp(name, "ingest_times")) {
        if (!dst || max_bytes < (int64_t)sizeof ctx->ingest_ms) return CPOL_ERR_ARG;
        memcpy(dst, ctx->ingest_ms, sizeof ctx->ingest_ms);
        return (int64_t)sizeof ctx->ingest_ms;
    }
    if (!strcmp(name, "model_v") || !strcmp(name, "model_h") || !strcmp(name, "model_ht")) {
        // the staged model as it lies in device memory
        const cpol_ctx *own = ctx->parent ? ctx->parent : ctx;
        if (!own->model_staged) { ctx->err = "cpol_debug_read: no model staged"; return CPOL_ERR_ARG; }
        const ModelDev &md = own->model;
        const int64_t ncell = (int64_t)md.ny * md.nx;
        const void *from = name[6] == 'v' ? (const void *)md.V : name[7] == 't' ? (const void *)md.HT : (const void *)md.H;
        const int64_t nb = name[6] == 'v' ? ncell * md.nz * md.n_vars * 4 : name[7] == 't' ? ncell * 8 : ncell * md.nz * 4;
        if (!dst || nb > max_bytes) { ctx->err = "cpol_debug_read: destination too small"; return CPOL_ERR_ARG; }
        if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(dst, from, (size_t)nb, hipMemcpyDeviceToHost) != hipSuccess) {
            ctx->err = "cpol_debug_read: copy failed";
            return CPOL_ERR_HIP;
        }
        return nb;
    }
    if (!strcmp(name, "cache")) {
        // [integral-table cache entries, scattering-table cache entries, integral-table builds] (table_id)
        const cpol_ctx *own = ctx->parent ? ctx->parent : ctx;
        const double v[3] = {(double)own->itab_cache.size(), (double)own->table_cache.size(), (double)own->itab_builds};
        if (!dst || max_bytes < (int64_t)sizeof v) return CPOL_ERR_ARG;
        memcpy(dst, v, sizeof v);
        return (int64_t)sizeof v;
    }
    if (!strncmp(name, "itab_detail", 11) && name[11] >= '0' && name[11] < '0' + CPOL_MAX_HYDRO && !name[12]) {
        // slot j ("itab_detail<j>"): log2_lo, panels per octave, d0, n_pan, then the worst deviation at the
        // check points per function (CPOL_ITAB_NF values), per lambda panel (n_pan values: both check points;
        // n_pan values: the point near the panel edge alone), the accepted run of panels [lo, hi); 1-D tables only
        const cpol_ctx *own = ctx->parent ? ctx->parent : ctx;
        const std::vector<double> &v = own->itab_detail[name[11] - '0'];
        const int64_t nb = (int64_t)(v.size() * sizeof(double));
        if (!dst || max_bytes < nb) return nb ? -nb - 1000 : 0;      // (size query: -(bytes) - 1000)
        if (nb) memcpy(dst, v.data(), (size_t)nb);
        return nb;
    }
#ifdef CPOL_SUBSUM_STATS
    if (!strcmp(name, "subsum_stats")) {
        if (!dst || max_bytes < 32) return CPOL_ERR_ARG;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_subsum_stats), 32));
        unsigned long long z[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_subsum_stats), z, 32));
        return 32;
    }
#endif
#ifdef CPOL_RARE_TRACE
    if (!strcmp(name, "rare_trace")) {
        if (!dst || max_bytes < 64 * 8 * 8) return CPOL_ERR_ARG;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_rare_trace), 64 * 8 * 8));
        return 64 * 8 * 8;
    }
#endif
#if defined(CPOL_SUBSUM_TRACE) || defined(CPOL_LOOKUP_TRACE) || defined(CPOL_INTERP_TRACE)
    if (!strcmp(name, "subsum_trace")) {
        const int64_t nb = (int64_t)sizeof(unsigned long long) * CPOL_SUBSUM_TRACE_W * CPOL_SUBSUM_TRACE_N;
        if (!dst || max_bytes < nb) return CPOL_ERR_ARG;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_subsum_trace), (size_t)nb));
        return nb;
    }
#endif
    if (!strcmp(name, "itab_times")) {
        // per hydrometeor slot: device ms of the last integral-table build, and of its accuracy check
        const cpol_ctx *own = ctx->parent ? ctx->parent : ctx;
        if (!dst || max_bytes < (int64_t)sizeof own->itab_ms) return CPOL_ERR_ARG;
        memcpy(dst, own->itab_ms, sizeof own->itab_ms);
        return (int64_t)sizeof own->itab_ms;
    }
    if (!strcmp(name, "itab_check")) {
        // per hydrometeor slot: worst |polynomial - integrating kernel| / scale over the check points of its
        // integral table (1-D and 2-D); negative: table rejected (the slot is integrated bin by bin);
        // 0: no table.  Then (optional) where, and the number of (block, function) pairs above the limit
        const cpol_ctx *own = ctx->parent ? ctx->parent : ctx;
        if (!dst || max_bytes < (int64_t)sizeof own->itab_check) return CPOL_ERR_ARG;
        memcpy(dst, own->itab_check, sizeof own->itab_check);
        if (max_bytes >= 4 * (int64_t)sizeof own->itab_check) {
            memcpy((char *)dst + sizeof own->itab_check, own->itab_check_at, sizeof own->itab_check_at);
            memcpy((char *)dst + 2 * sizeof own->itab_check, own->itab_bad, sizeof own->itab_bad);
            memcpy((char *)dst + 3 * sizeof own->itab_check, own->itab_check_edge, sizeof own->itab_check_edge);
            return 4 * (int64_t)sizeof own->itab_check;
        }
        if (max_bytes >= 3 * (int64_t)sizeof own->itab_check) {
            memcpy((char *)dst + sizeof own->itab_check, own->itab_check_at, sizeof own->itab_check_at);
            memcpy((char *)dst + 2 * sizeof own->itab_check, own->itab_bad, sizeof own->itab_bad);
            return 3 * (int64_t)sizeof own->itab_check;
        }
        if (max_bytes >= 2 * (int64_t)sizeof own->itab_check) {
            memcpy((char *)dst + sizeof own->itab_check, own->itab_check_at, sizeof own->itab_check_at);
            return 2 * (int64_t)sizeof own->itab_check;
        }
        return (int64_t)sizeof own->itab_check;
    }
    if (!dst || ctx->last_n_sbg <= 0) return CPOL_ERR_ARG;
    const long n_sbg = ctx->last_n_sbg, n_rg = ctx->last_n_rg;
    const int n_hyd = ctx->hs.n_hydro, n_vars = ctx->model.n_vars;
    const void *src = nullptr;
    int64_t bytes = 0;
    if (!strcmp(name, "sub_values")) { src = ctx->b_vals.p; bytes = (int64_t)n_vars * n_sbg * 4; }
    else if (!strcmp(name, "sub_mask")) { src = ctx->b_mask.p; bytes = n_sbg; }
    else if (!strcmp(name, "sub_elev")) { src = ctx->b_elev.p; bytes = n_sbg * 4; }
    else if (!strcmp(name, "sub_coords")) { src = ctx->b_coords.p; bytes = n_sbg * 8; }
    else if (!strcmp(name, "sub_wgate")) { src = ctx->b_wgate.p; bytes = n_sbg * 8; }      // integration scheme 'ml': per-gate weights of every sub-beam
    else if (!strcmp(name, "item_key")) { src = ctx->b_key.p; bytes = (int64_t)n_hyd * n_sbg * 4; }
    else if (!strcmp(name, "item_res")) {
        if (ctx->last_subsum) {
            ctx->err = "cpol_debug_read: item_res is incomplete (the items on 1-D integral tables are evaluated inside "
                       "k_subbeam_sum / k_final and never stored; CPOL_SUBSUM=0 keeps them)";
            return CPOL_ERR_ARG;
        }
        src = ctx->b_res.p; bytes = (int64_t)n_hyd * n_sbg * CPOL_N_SZ * 8;
    }
    else if (!strcmp(name, "item_vmask")) {
        // the validity bits of every sub-beam gate (bit j: hydrometeor j present)
        if (!ctx->last_vmask) {
            ctx->err = "cpol_debug_read: item_vmask is incomplete (the single-beam kernels write it only where a species' fall-speed sums "
                       "are totals over the ray; debug reads or CPOL_GATE1=0 keep the general launch sequence)";
            return CPOL_ERR_ARG;
        }
        src = ctx->b_vmask.p; bytes = n_sbg;
    }
    else if (!strcmp(name, "item_vn")) {
        // the fall-speed moments {v, n} of every item (defined where the item's bit of item_vmask is set)
        if (!ctx->last_vn) {
            ctx->err = "cpol_debug_read: item_vn is incomplete (read back for every sub-beam gate only under Doppler scheme 1 in the general "
                       "launch sequence: the single-beam kernels keep the moments in registers; debug reads or CPOL_GATE1=0 keep them)";
            return CPOL_ERR_ARG;
        }
        src = ctx->b_vn.p; bytes = (int64_t)n_hyd * n_sbg * 2 * 8;
    }
    else if (!strcmp(name, "ice_first")) {
        // one record {int32 first_gate, int32 pad, float64 v, float64 n} per (ray, sub-beam) (k_ice_first)
        if (!ctx->last_icefirst) {
            ctx->err = "cpol_debug_read: ice_first is not written (k_ice_first runs under Doppler scheme 1 in the general launch sequence "
                       "when a species' fall-speed sums are totals over the ray: 1-moment ice, numeric integrate_V)";
            return CPOL_ERR_ARG;
        }
        src = ctx->b_icefirst.p; bytes = (int64_t)ctx->last_n_rays * ctx->last_n_sub * (int64_t)sizeof(IceFirst);
    }
    else if (!strcmp(name, "item_rec")) { src = ctx->b_rec.p; bytes = (int64_t)n_hyd * n_sbg * 16; }
    else if (!strcmp(name, "item_par")) { src = ctx->b_par.p; bytes = (int64_t)n_hyd * CPOL_MAX_PAR * n_sbg * 8; }
    else if (!strcmp(name, "q_melt")) { src = ctx->b_qmelt.p; bytes = 2 * n_sbg * 4; }
    else if (!strcmp(name, "fw_melt")) { src = ctx->b_fwmelt.p; bytes = 2 * n_sbg * 8; }
    else if (!strcmp(name, "sz_integ")) { src = ctx->b_szinteg.p; bytes = (int64_t)n_rg * n_hyd * CPOL_N_SZ * 4; }
    else if (!strcmp(name, "sz_total")) { src = ctx->b_sztotal.p; bytes = (int64_t)n_rg * CPOL_N_SZ * 4; }
    else if (!strcmp(name, "traj")) { src = ctx->b_traj.p; bytes = (int64_t)ctx->last_n_rays * ctx->last_n_v * 3 * ctx->last_n_gates * 4; }
    else if (!strcmp(name, "geo_poly")) {
        // the coordinate polynomials of the last sweep, float64 [n_rays][n_h][2][CPOL_GEO_NP] monomial coefficients in x (NaN: a fit that
        // k_trajectory's sanity rules rejected); a test hook like cpol_debug_math
        if (!ctx->last_poly) { ctx->err = "cpol_debug_read: the last sweep took no coordinate polynomials"; return CPOL_ERR_ARG; }
        src = ctx->last_poly; bytes = (int64_t)ctx->last_poly_fits * 2 * CPOL_GEO_NP * 8;
    }
    else if (!strcmp(name, "psd_clock")) { src = ctx->b_clk.p; bytes = 2048 * 4 * 8; }
    else if (!strcmp(name, "bucket_count")) { src = (const int *)ctx->b_count.p + ctx->last_par * ctx->count_stride; bytes = (int64_t)ctx->last_n_keys * 4; }
    else { ctx->err = std::string("cpol_debug_read: unknown buffer ") + name; return CPOL_ERR_ARG; }
    if (!src) { ctx->err = "cpol_debug_read: buffer not kept (call with name \"enable\" first)"; return CPOL_ERR_ARG; }
    if (bytes > max_bytes) { ctx->err = "cpol_debug_read: destination too small"; return CPOL_ERR_ARG; }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        ctx->err = "cpol_debug_read: copy failed";
        return CPOL_ERR_HIP;
    }
    return bytes;
}

}  // extern "C"
