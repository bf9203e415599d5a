// cpol_buffers.h -- which device work buffers a sweep needs and how large: every per-sweep work buffer of the context that
// run_sequence (cosmo_pol_hip.hip) sizes, decided once per call by plan_buffers() from plain numbers and the call's Forms.
// Plain C++ without HIP types, so that a host test can include it (tests/c_host/buffers_check.cpp, tests/test_buffers_cpu.py
// pin the sizes without a GPU).  The table BUF_ROWS below is what cpol_mem_info, cpol_destroy, the fills on replacement and
// the graph key walk; the slack of a grow-only buffer stays in ensure(), the bases and the order of the fills in run_sequence.
#pragma once

#include <cstddef>
#include "cpol_forms.h"

// build constants of the kernel files that the sizes read (cosmo_pol_hip.hip asserts each against its kernel file)
constexpr int BUF_GEO_NP = 9;                  // CPOL_GEO_NP (cpol_interp.inl)
constexpr int BUF_MAX_PAR = 6;                 // CPOL_MAX_PAR (cpol_psd.inl)
constexpr int BUF_COUNT_SLOTS = 1024;          // CPOL_COUNT_SLOTS (cpol_psd.inl)
constexpr int BUF_ICEFIRST_BYTES = 24;         // sizeof(IceFirst) (cpol_final.inl)
constexpr int BUF_WORKUNIT_BYTES = 16;         // sizeof(WorkUnit) (cpol_device.h)
constexpr int BUF_CLK_BYTES = 2048 * 4 * 8;    // the clock probe of the PSD stage (cpol_debug_read "psd_clock")
constexpr int BUF_MAX_COLS = CPOL_MAX_VARS + 6;        // the inputs of a columns call: the variables, then mask, elev, wgate, q_melt, fw_melt, has_melting

enum WorkBuf {
    WB_TRAJ, WB_RAYC, WB_POLY, WB_TIMED, WB_VALS, WB_MASK, WB_ELEV, WB_COORDS, WB_WGATE, WB_QMELT, WB_FWMELT,
    WB_KEY, WB_POS, WB_PAR, WB_COUNT, WB_TOTALS, WB_BLKRANKED, WB_REC, WB_VMASK, WB_OFFSET, WB_PERM, WB_RES,
    WB_VN, WB_ICEFIRST, WB_PROJ, WB_COLIN, WB_XSCR, WB_XGEO, WB_BEAM, WB_BSIGMA, WB_BON,
    WB_GSCAN, WB_DEFER, WB_PRESENT, WB_TICKET, WB_UNITS, WB_SZINTEG, WB_CLK, WB_N
};

enum BufFill { FILL_NONE = 0, FILL_ZERO, FILL_FF };

// One row per work buffer.  gate / per_var / per_hyd: its bytes per sub-beam gate = gate + per_var * n_vars + per_hyd * n_hydro
// (all 0: it does not scale that way, plan_buffers states its size); per_gate: counted in cpol_mem_info's bytes per sub-beam gate;
// held: counted in cpol_mem_info's "held already"; fill: what run_sequence queues when ensure() replaced it
struct BufRow {
    int gate, per_var, per_hyd;
    bool per_gate, held;
    BufFill fill;
};

constexpr BufRow BUF_ROWS[WB_N] = {
    /* traj      */ {0, 0, 0, false, true, FILL_NONE},
    /* rayc      */ {0, 0, 0, false, true, FILL_NONE},
    /* poly      */ {0, 0, 0, false, false, FILL_NONE},
    /* timed     */ {0, 0, 0, false, false, FILL_NONE},
    /* vals      */ {0, 4, 0, true, true, FILL_NONE},
    /* mask      */ {1, 0, 0, true, true, FILL_NONE},
    /* elev      */ {4, 0, 0, true, true, FILL_NONE},
    /* coords    */ {8, 0, 0, false, true, FILL_NONE},
    /* wgate     */ {8, 0, 0, true, true, FILL_NONE},
    /* qmelt     */ {8, 0, 0, true, true, FILL_NONE},
    /* fwmelt    */ {16, 0, 0, true, true, FILL_NONE},
    /* key       */ {0, 0, 4, true, true, FILL_NONE},
    /* pos       */ {0, 0, 4, true, true, FILL_NONE},
    /* par       */ {0, 0, BUF_MAX_PAR * 8, true, true, FILL_NONE},
    /* count     */ {0, 0, 0, false, false, FILL_ZERO},          // (both counter sets together: see run_sequence)
    /* totals    */ {0, 0, 0, false, false, FILL_ZERO},
    /* blkranked */ {0, 0, 0, false, false, FILL_NONE},
    /* rec       */ {0, 0, 16, true, true, FILL_NONE},
    /* vmask     */ {1, 0, 0, true, true, FILL_NONE},
    /* offset    */ {0, 0, 0, false, false, FILL_NONE},
    /* perm      */ {0, 0, 4, true, true, FILL_NONE},
    /* res       */ {0, 0, CPOL_N_SZ * 8, true, true, FILL_NONE},
    /* vn        */ {0, 0, 16, true, true, FILL_NONE},
    /* icefirst  */ {0, 0, 0, false, false, FILL_NONE},
    /* proj      */ {8, 0, 0, true, true, FILL_NONE},
    /* colin     */ {0, 0, 0, false, false, FILL_NONE},
    /* xscr      */ {0, 0, 0, false, false, FILL_NONE},
    /* xgeo      */ {0, 0, 0, false, false, FILL_NONE},
    /* beam      */ {0, 0, 0, false, true, FILL_NONE},
    /* bsigma    */ {8, 0, 0, false, false, FILL_NONE},
    /* bon       */ {0, 0, 0, false, false, FILL_NONE},
    /* gscan     */ {0, 0, 0, false, true, FILL_NONE},
    /* defer     */ {0, 0, 0, false, true, FILL_NONE},
    /* present   */ {0, 0, 0, false, false, FILL_FF},          // ("anything may be here" until k_interp_sweep has written the word)
    /* ticket    */ {0, 0, 0, false, false, FILL_ZERO},         // (k_gate1_ray_scan leaves every ticket at 0 behind it)
    /* units     */ {0, 0, 0, false, true, FILL_NONE},
    /* szinteg   */ {0, 0, 0, false, true, FILL_NONE},
    /* clk       */ {0, 0, 0, false, false, FILL_NONE},
};

inline size_t buf_gate_bytes(int w, size_t n_vars, size_t n_hydro)
{
    return (size_t)BUF_ROWS[w].gate + (size_t)BUF_ROWS[w].per_var * n_vars + (size_t)BUF_ROWS[w].per_hyd * n_hydro;
}

// cpol_mem_info: the work-buffer bytes per sub-beam gate of a launch sequence
inline size_t buf_per_gate(size_t n_vars, size_t n_hydro)
{
    size_t sum = 0;
    for (int w = 0; w < WB_N; ++w) if (BUF_ROWS[w].per_gate) sum += buf_gate_bytes(w, n_vars, n_hydro);
    return sum;
}

// ---- what the sizes read ----
struct BufIn {
    int n_rays = 0, n_gates = 0, n_sub = 0, n_h = 0, n_v = 0, n_vars = 0, n_hydro = 0, n_keys = 0, n_vbins = 0;
    int mode = 0;                              // cpol_sweep_params.geometry_mode
    bool keep_debug = false, ml = false, doppler = false, dop3 = false, broaden = false, timed = false;
    bool columns = false, inputs_on_device = false;
    bool col_given[6] = {false, false, false, false, false, false};    // mask, elev, wgate, q_melt, fw_melt, has_melting as the call reads them
    bool sub_export = false;
    bool want_species = false;                 // cpol_outputs.species: k_species reads the per-species rows
    int classify_threads = 0;                 // CPOL_CLASSIFY_THREADS of the build
    bool present_words = false;                // CPOL_GATE1_PRESENT of the build
    Forms f;
};

// ---- what they decide ----
struct BufPlan {
    size_t bytes[WB_N] = {};                   // exactly what the call asks for; 0: not needed
    long cnt_stride = 0;                       // ints per counter set: [n_keys] bucket counts, [n_keys + 2] items ranked, [n_keys + 3 ...) items on integral tables
    long unit_cap = 0;                         // work units of the PSD stage: up to 64 / 128 sorted items each, or one per item (virtual: no b_units entries)
    int n_col = 0;                             // columns: the inputs in the order k_columns_ingest takes them, their bytes and where the
    size_t col_bytes[BUF_MAX_COLS] = {};       // host ones are staged inside b_colin (each padded to 256 bytes)
    size_t col_off[BUF_MAX_COLS] = {};
    size_t xscr_mask = 0, xscr_elev = 0;       // sub-beam export: b_xscr holds the values (at 0), the mask and the elevation of the long-form gate kernel
    size_t xgeo_lons = 0, xgeo_dist = 0, xgeo_heights = 0, xgeo_elev = 0, xgeo_mlmask = 0;      // ... b_xgeo lats (at 0), lons, dist, heights, elev, mask_ml
};

inline BufPlan plan_buffers(const BufIn &in)
{
    BufPlan pl;
    const Forms &f = in.f;
    const size_t n_rays = (size_t)in.n_rays, ng = (size_t)in.n_gates, n_sub = (size_t)in.n_sub, n_h = (size_t)in.n_h, n_v = (size_t)in.n_v;
    const size_t n_vars = (size_t)in.n_vars, n_hyd = (size_t)in.n_hydro, n_keys = (size_t)in.n_keys, n_vb = (size_t)in.n_vbins;
    const size_t n_rg = n_rays * ng, n_sbg = n_rg * n_sub;
    const auto pad256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t *const b = pl.bytes;
    // every buffer that holds a fixed number of bytes per sub-beam gate (the rows of the table), where the call needs it
    const auto per_gate = [&](int w) { b[w] = buf_gate_bytes(w, n_vars, n_hyd) * n_sbg; };
    for (int w : {WB_VALS, WB_MASK, WB_ELEV, WB_QMELT, WB_FWMELT, WB_KEY, WB_POS, WB_PAR, WB_REC, WB_VMASK, WB_PERM, WB_RES}) per_gate(w);
    if (in.keep_debug) per_gate(WB_COORDS);
    if (in.ml) per_gate(WB_WGATE);
    if (in.doppler) per_gate(WB_VN);
    if (in.doppler && f.rvel_terms) per_gate(WB_PROJ);
    if (in.dop3 && in.broaden) per_gate(WB_BSIGMA);
    // the ray paths, the per-ray constants and the coordinate polynomials of k_trajectory; the brackets of a time-blended call
    if (in.mode == CPOL_GEOM_HOST_PATHS || in.keep_debug || f.prep_paths) b[WB_TRAJ] = n_rays * n_v * 3 * ng * sizeof(float);
    if (f.ray_prep) b[WB_RAYC] = (n_rays * n_h + n_rays) * 2 * sizeof(double);
    if (f.geo_poly) b[WB_POLY] = n_rays * n_h * 2 * BUF_GEO_NP * sizeof(double);
    if (in.timed) b[WB_TIMED] = 2 * n_rays * sizeof(int);
    // the two counter sets, the ranking and the work units of the PSD stage
    pl.cnt_stride = (long)n_keys + 3 + BUF_COUNT_SLOTS;
    b[WB_COUNT] = 2 * (size_t)pl.cnt_stride * sizeof(int);
    b[WB_TOTALS] = 2 * 4 * sizeof(long long);
    b[WB_BLKRANKED] = (n_sbg + (size_t)in.classify_threads - 1) / (size_t)in.classify_threads * sizeof(int);
    b[WB_OFFSET] = 2 * n_keys * sizeof(int);                 // item and unit offsets
    pl.unit_cap = f.rare_direct ? (long)(n_hyd * n_sbg) : (long)(n_hyd * n_sbg / 64 + n_keys + 64);
    if (!f.rare_direct) b[WB_UNITS] = (size_t)pl.unit_cap * BUF_WORKUNIT_BYTES;
    if (in.doppler) b[WB_ICEFIRST] = n_rays * n_sub * BUF_ICEFIRST_BYTES;
    // columns: where k_columns_ingest reads each input (host inputs: a device staging area, one copy per array)
    if (in.columns) {
        for (size_t v = 0; v < n_vars; ++v) pl.col_bytes[pl.n_col++] = n_sbg * sizeof(float);
        const size_t rest[6] = {n_sbg, n_sbg * sizeof(float), n_sbg * sizeof(double), 2 * n_sbg * sizeof(float), 2 * n_sbg * sizeof(double),
                                n_rays * n_sub};
        for (int k = 0; k < 6; ++k) pl.col_bytes[pl.n_col++] = in.col_given[k] ? rest[k] : 0;
        size_t total = 0;
        for (int k = 0; k < pl.n_col; ++k) { pl.col_off[k] = total; total += pad256(pl.col_bytes[k]); }
        if (!in.inputs_on_device) b[WB_COLIN] = total;
    }
    // sub-beam export: the long-form gate kernel's own values / mask / elevation (scratch), the geometry of every sub-beam
    // (lats, lons, dist, heights, elev) and mask_ml
    if (in.sub_export) {
        const size_t xa8 = pad256(n_sbg * sizeof(double)), xa4 = pad256(n_sbg * sizeof(float)), xa1 = pad256(n_sbg);
        pl.xscr_mask = n_vars * xa4; pl.xscr_elev = pl.xscr_mask + xa1;
        b[WB_XSCR] = pl.xscr_elev + xa4;
        pl.xgeo_lons = xa8; pl.xgeo_dist = 2 * xa8; pl.xgeo_heights = pl.xgeo_dist + xa4; pl.xgeo_elev = pl.xgeo_heights + xa4;
        pl.xgeo_mlmask = pl.xgeo_elev + xa4;
        b[WB_XGEO] = pl.xgeo_mlmask + xa1;
    }
    // Doppler scheme 3: the spectrum of every sub-beam gate, the switch of the broadening per (ray, sub-beam)
    if (in.dop3) {
        b[WB_BEAM] = n_sbg * n_vb * sizeof(float);
        if (in.broaden) b[WB_BON] = n_rays * n_sub * sizeof(int);
    }
    // the single-beam kernels: the range scans' terms, the presence words, the tickets of the rays
    if (f.gate1) { b[WB_GSCAN] = 3 * n_rg * sizeof(float); b[WB_DEFER] = n_rg; }
    if (f.gate1_ray && in.present_words) b[WB_PRESENT] = n_rays * ((ng + 63) / 64) * sizeof(unsigned);
    if (f.gate1_ray && f.g1r == 3) b[WB_TICKET] = n_rays * sizeof(int);
    if (in.keep_debug || f.subsum || in.want_species) b[WB_SZINTEG] = n_rg * n_hyd * CPOL_N_SZ * sizeof(float);
    if (in.keep_debug && !in.sub_export) b[WB_CLK] = BUF_CLK_BYTES;      // (the export stops before the PSD stage)
    return pl;
}

// the work buffers whose pointers the graph key mixes: every one the call sized, in the order of the enum
inline int buf_key_list(const BufPlan &pl, int list[WB_N])
{
    int n = 0;
    for (int w = 0; w < WB_N; ++w) if (pl.bytes[w]) list[n++] = w;
    return n;
}
