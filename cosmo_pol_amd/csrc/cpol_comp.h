// cpol_comp.h -- gridded composites (cpol_composite): every refusal, the rounding of the slab and the thresholds to float32, the
// plane list, the plane (radar-centred or the caller's per-gate coordinates), the source, the layout of the running state (with
// SOURCE: its source bytes and the per-call scratch behind it) and the block arithmetic of a call, decided by comp_check() from
// plain numbers.
// Plain C++ without HIP types, so that a host program can include it (tests/c_host/comp_check.cpp, tests/test_composite_cpu.py
// check it without a GPU; comp_check_network.cpp, test_composite_network_cpu.py the network additions; comp_check_layers.cpp,
// test_composite_layers_cpu.py the height layers and the column).  The kernels are k_comp,
// k_comp_merge, k_comp_finish and k_comp_column (cpol_comp.inl); the rule is stated in
// include/cosmo_pol_amd.h and cosmo_pol_amd/composite.py.  The exact sums (CPOL_COMP_SUM, cpol_composite_sums: the tail's
// refusals, the bins of the state, the gates a pass may fold) are checked by comp_check_sums.cpp, test_composite_sums_cpu.py;
// their kernels are k_comp_sum and k_comp_sum_finish.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cpol_hist.h"

constexpr int COMP_FIELDS = CPOL_COMP_FIELDS;
constexpr int COMP_MAX_THR = CPOL_COMP_MAX_THRESHOLDS;
constexpr int COMP_MAX_EDGES = HIST_MAX_EDGES;     // n + 1 of either axis: both axes' float64 edges fit 16 KiB of LDS
constexpr long COMP_MAX_STATE_BYTES = 1L << 30;    // the state of all blocks and fields
// gates per workgroup of k_comp: a workgroup reads both axes' edges into LDS once (4.8 KB for a 300 x 300 grid), so a stretch
// is long enough for its own 12 KB of gates to outweigh them; the 180 000 gates of a 360 x 500 sweep give 176 workgroups
constexpr int COMP_STRETCH = 1024;
constexpr int COMP_THREADS = 256;                  // threads of a workgroup of k_comp and k_comp_finish
constexpr uint32_t COMP_PRODUCTS = CPOL_COMP_MAX | CPOL_COMP_LOWEST | CPOL_COMP_ECHO_TOP | CPOL_COMP_SOURCE | CPOL_COMP_COLUMN | CPOL_COMP_SUM;
constexpr int COMP_MAX_LAYERS = CPOL_COMP_MAX_LAYERS;      // n_z: the float32 layer edges (at most 65) lie in LDS beside the x and y edges
constexpr int COMP_MAX_TABLE = CPOL_COMP_MAX_TABLE;        // breakpoints of a column table: 4 KB + 8 KB of LDS in k_comp_column
constexpr size_t COMP_TAB_EDGE_WORDS = 40;                 // float64 words at the head of the device's table block: room for the 65 float32 layer edges
constexpr int COMP_NO_SOURCE = 255;               // the begin value of a source byte: no call has set the cell
// ---- the exact sums (CPOL_COMP_SUM).  A finite float32 is  +-M * 2^(E - 150)  with E in 1 ... 254 and M < 2^24 (obj_sum_split,
// cpol_obj.h).  THE ROW of a (block, layer, cell) and field: COMP_SUM_BINS signed 64-bit bins (two's complement, added as unsigned
// long long); bin E >> 3 takes  +-M << (E & 7): the moment layout of cpol_obj.h with the multiplier 1, so obj_sum_round(row, 32, 8)
// finishes a row unchanged.  NO OVERFLOW, a condition and not a measurement: a term is below 2^24 * 2^7 = 2^31 in magnitude, so
// after n terms |bin| < n * 2^31, which is below 2^63 while n < 2^32: a bin cannot wrap while fewer than 2^32 gates fold into one
// block of a pass.  CompPass keeps the gates folded per block so far, and comp_check refuses the call that would take them beyond
// COMP_SUM_MAX_GATES.  The sum of a row is below 2^(8 * 31 + 63) = 2^311 in magnitude (in units of 2^-150): the 384 bits of
// obj_sum_round hold it with its sign.  (k_comp_sum combines at most 64 terms of a wavefront before the atomic: below 2^37.) ----
constexpr int COMP_SUM_BINS = 32;
constexpr int COMP_SUM_ROW_BYTES = COMP_SUM_BINS * 8;
constexpr unsigned long long COMP_SUM_MAX_GATES = 0xFFFFFFFFull;      // 2^32 - 1 gates per block of a pass

// what the entry point knows of the call
struct CompCall {
    long n_rows = 0;               // n_rays, or n_members * n_rays
    int n_gates = 0;
    bool spaceborne = false;       // per-ray radar positions: no one plane holds the gates
};

// the open pass of a context (the states themselves live on the device)
struct CompPass {
    bool open = false;
    uint32_t fields = 0, products = 0;
    int plane = 0;
    long n_blocks = 0;
    bool slab = false;
    float h_lo = 0.f, h_hi = 0.f;
    std::vector<float> thr[COMP_FIELDS];           // the ROUNDED thresholds
    std::vector<double> ex, ey;
    // height layers and the column: the ROUNDED layer edges (empty: none), gaps, and per field the table as the begin found it
    std::vector<float> ez;
    int gaps = 0;
    std::vector<float> tv[COMP_FIELDS];
    std::vector<double> tf[COMP_FIELDS];
    // the exact sums: per field the weight table as the begin found it (empty: w = v), and the gates folded into one block so far
    std::vector<float> wv[COMP_FIELDS];
    std::vector<double> wf[COMP_FIELDS];
    unsigned long long sum_gates = 0;
};

// a call that passed: the numbers the launches need
struct CompPlan {
    int n_fields = 0;
    int field[COMP_FIELDS] = {};                   // the requested fields, ascending
    int slot[COMP_FIELDS] = {};                    // field k's row of `count`
    int n_thr[COMP_FIELDS] = {};
    int n_planes[COMP_FIELDS] = {};                // of values[k]: 2 (MAX) + 2 (LOWEST) + n_thr, with SOURCE one more per MAX and LOWEST
    int n_x = 0, n_y = 0;
    long cells = 0;                                // n_x * n_y
    uint32_t products = 0;
    bool slab = false;
    float h_lo = 0.f, h_hi = 0.f;
    std::vector<float> thr[COMP_FIELDS];
    std::vector<double> ex, ey;
    long n_blocks = 1, rows_per_block = 0;
    // the state, in bytes: first what a begin sets to 0 -- per field the MAX states (uint64 [n_blocks][cells]), the counts
    // (likewise) and the echo-top states (uint32 [n_blocks][n_thr][cells], padded to 8 bytes) -- then what it sets to all ones:
    // per field the LOWEST states (uint64 [n_blocks][cells]).  -1: the field has none
    long off_max[COMP_FIELDS] = {}, off_count[COMP_FIELDS] = {}, off_top[COMP_FIELDS] = {}, off_low[COMP_FIELDS] = {};
    long zero_bytes = 0, state_bytes = 0;
    // behind the running state, with SOURCE alone: the source bytes (uint8 [n_blocks][cells] per field and product, begin value
    // 255, each padded to 8 bytes: -1 the field has none), then the per-call scratch state, state_bytes with the offsets and the
    // begin values of the running state.  total_bytes = state_bytes without SOURCE: what the 1 GiB limit counts
    long off_src_max[COMP_FIELDS] = {}, off_src_low[COMP_FIELDS] = {};
    long off_scratch = -1, total_bytes = 0;
    int plane = 0, source = 0;
    bool with_source = false;
    bool begin = false, finish = false;
    // height layers and the column: n_z = 0 none -- else a block of every state holds n_z * cells entries (block_cells), and
    // k_comp_finish serves n_blocks * n_z blocks of `cells`
    int n_z = 0, gaps = 0;
    long block_cells = 0;                          // max(n_z, 1) * cells
    bool column = false;
    std::vector<float> ez;                         // the ROUNDED layer edges [n_z + 1]
    std::vector<float> tv[COMP_FIELDS];            // the tables (empty: no column of the field)
    std::vector<double> tf[COMP_FIELDS];
    // the exact sums (CPOL_COMP_SUM): in the part of the state that a begin sets to 0, behind the field's echo-top states, the
    // rows of bins (int64 [n_blocks * block_cells][COMP_SUM_BINS]) and the skipped words (uint32 [n_blocks * block_cells], padded
    // to 8 bytes); -1: off.  wv, wf: the weight tables (empty: w = v); sum_gates: the gates of a block once this call is folded
    bool sum = false;
    long off_sum[COMP_FIELDS] = {}, off_skip[COMP_FIELDS] = {};
    std::vector<float> wv[COMP_FIELDS];
    std::vector<double> wf[COMP_FIELDS];
    unsigned long long sum_gates = 0;
};

// a threshold or slab bound rounded once to float32 (at or beyond the midpoint between FLT_MAX and 2^128: infinity, as IEEE rounds)
inline float comp_f32(double v)
{
    if (std::fabs(v) >= 0x1.ffffffp+127) return std::copysign(HUGE_VALF, (float)std::copysign(1.0, v));
    return (float)v;
}

// every refusal of a cpol_composite for a call; NULL: accepted and *pl filled; else the reason (CPOL_ERR_ARG).  Touches neither
// the pass nor anything else: the caller opens / closes the pass once the call is queued.
inline const char *comp_check(const cpol_composite *c, const CompCall &call, const CompPass &pass, CompPlan *pl)
{
    *pl = CompPlan{};
    if (call.spaceborne) return "a spaceborne call (per-ray radar positions) has no radar-centred plane";
    if (c->phase < 0 || c->phase > 3) return "phase must lie in 0 ... 3";
    if (((c->fields >> COMP_FIELDS) & 1u)) return "RVEL is float64 and is not composed";
    if (c->fields == 0 || (c->fields >> COMP_FIELDS) != 0) return "fields must name at least one of the 9 float32 fields and no other bit";
    if (c->products == 0 || (c->products & ~COMP_PRODUCTS) != 0)
        return "products must name MAX, LOWEST or ECHO_TOP and no other bit (beside them SOURCE, or COLUMN with height layers)";
    if (c->plane != CPOL_COMP_PLANE_RADAR && c->plane != CPOL_COMP_PLANE_GATES) return "plane must be CPOL_COMP_PLANE_RADAR or CPOL_COMP_PLANE_GATES";
    if (c->source < 0 || c->source >= COMP_NO_SOURCE) return "source must lie in 0 ... 254";
    pl->with_source = (c->products & CPOL_COMP_SOURCE) != 0;
    if (c->source != 0 && !pl->with_source) return "a non-zero source without SOURCE";
    if (pl->with_source && !(c->products & (CPOL_COMP_MAX | CPOL_COMP_LOWEST))) return "products: SOURCE needs MAX or LOWEST";
    // the exact sums: only with the bit is *c the first member of a cpol_composite_sums, and only then is anything behind it read
    pl->sum = (c->products & CPOL_COMP_SUM) != 0;
    const cpol_composite_sums *const cs = pl->sum ? (const cpol_composite_sums *)c : nullptr;
    if (pl->sum && !(c->products & (CPOL_COMP_MAX | CPOL_COMP_LOWEST | CPOL_COMP_ECHO_TOP))) return "products: SUM stands beside MAX, LOWEST or ECHO_TOP";
    if (pl->sum && pl->with_source) return "products: SUM with SOURCE (the scratch-and-merge pass carries no sums)";
    pl->products = c->products;
    pl->plane = c->plane; pl->source = c->source;
    const bool tops = (c->products & CPOL_COMP_ECHO_TOP) != 0;
    for (int k = 0; k < COMP_FIELDS; ++k) {
        if (!((c->fields >> k) & 1u)) continue;
        const int nt = c->n_thresholds[k];
        if (tops && (nt < 1 || nt > COMP_MAX_THR)) return "ECHO_TOP needs 1 ... 4 thresholds for every requested field";
        if (!tops && nt != 0) return "thresholds without ECHO_TOP";
        pl->thr[k].resize((size_t)nt);
        for (int j = 0; j < nt; ++j) {
            const double t = c->thresholds[k][j];
            if (!(t == t)) return "a threshold is NaN";
            pl->thr[k][(size_t)j] = comp_f32(t);
        }
        pl->slot[k] = pl->n_fields;
        pl->field[pl->n_fields++] = k;
        pl->n_thr[k] = nt;
        const int per_product = (c->products & CPOL_COMP_SOURCE) ? 3 : 2;
        pl->n_planes[k] = ((c->products & CPOL_COMP_MAX) ? per_product : 0) + ((c->products & CPOL_COMP_LOWEST) ? per_product : 0) + nt;
    }
    if (c->use_slab) {
        pl->slab = true;
        pl->h_lo = comp_f32(c->h_lo);
        pl->h_hi = comp_f32(c->h_hi);
        if (!(pl->h_lo < pl->h_hi)) return "the height slab needs h_lo < h_hi after rounding to float32";
    }
    // height layers and the column
    if (c->n_z < 0 || c->n_z > COMP_MAX_LAYERS) return "n_z must lie in 0 ... 64";
    pl->n_z = c->n_z;
    pl->column = (c->products & CPOL_COMP_COLUMN) != 0;
    if (pl->column && c->n_z == 0) return "COLUMN needs height layers (n_z, edges_z)";
    if (pl->column && !(c->products & CPOL_COMP_MAX)) return "COLUMN needs MAX";
    if (c->gaps != CPOL_COMP_GAPS_ZERO && c->gaps != CPOL_COMP_GAPS_HOLD) return "gaps must be CPOL_COMP_GAPS_ZERO or CPOL_COMP_GAPS_HOLD";
    if (c->gaps != 0 && !pl->column) return "gaps without COLUMN";
    pl->gaps = c->gaps;
    if (c->n_z > 0) {
        if (c->use_slab) return "height layers with a height slab: the first and last edge are the slab";
        if (c->products & CPOL_COMP_LOWEST) return "height layers with LOWEST: per layer the maximum and the count alone";
        if (c->products & CPOL_COMP_ECHO_TOP) return "height layers with ECHO_TOP: per layer the maximum and the count alone";
        if (c->products & CPOL_COMP_SOURCE) return "height layers with SOURCE: per layer the maximum and the count alone";
        if (!c->edges_z) return "edges_z is NULL";
        pl->ez.resize((size_t)c->n_z + 1);
        for (int j = 0; j <= c->n_z; ++j) {
            if (!(c->edges_z[j] == c->edges_z[j])) return "a layer edge is NaN";
            pl->ez[(size_t)j] = comp_f32(c->edges_z[j]);
            if (j && !(pl->ez[(size_t)j - 1] < pl->ez[(size_t)j])) return "the layer edges are not strictly ascending after rounding to float32";
        }
    }
    {
        bool any_table = false;
        for (int k = 0; k < COMP_FIELDS; ++k) {
            const int n = c->n_table[k];
            if (n == 0) continue;
            if (!pl->column) return "a column table without COLUMN";
            if (!((c->fields >> k) & 1u)) return "a column table of a field that is not requested";
            if (n < 2 || n > COMP_MAX_TABLE) return "a column table needs 2 ... 1024 breakpoints";
            if (!c->table_v[k] || !c->table_f[k]) return "table_v or table_f is NULL";
            pl->tv[k].assign(c->table_v[k], c->table_v[k] + n);
            pl->tf[k].assign(c->table_f[k], c->table_f[k] + n);
            for (int j = 0; j < n; ++j) {
                if (!std::isfinite(pl->tv[k][(size_t)j]) || !std::isfinite(pl->tf[k][(size_t)j])) return "a breakpoint or a value of a column table is NaN or infinite";
                if (j && !(pl->tv[k][(size_t)j - 1] < pl->tv[k][(size_t)j])) return "the breakpoints of a column table are not strictly ascending";
            }
            any_table = true;
        }
        if (pl->column && !any_table) return "COLUMN needs a table for at least one requested field";
    }
    for (int k = 0; cs && k < COMP_FIELDS; ++k) {
        const int n = cs->n_weight[k];
        if (n == 0) continue;
        if (!((c->fields >> k) & 1u)) return "a weight table of a field that is not requested";
        if (n < 2 || n > COMP_MAX_TABLE) return "a weight table needs 2 ... 1024 breakpoints";
        if (!cs->weight_v[k] || !cs->weight_f[k]) return "weight_v or weight_f is NULL";
        pl->wv[k].assign(cs->weight_v[k], cs->weight_v[k] + n);
        pl->wf[k].assign(cs->weight_f[k], cs->weight_f[k] + n);
        for (int j = 0; j < n; ++j) {
            if (!std::isfinite(pl->wv[k][(size_t)j]) || !std::isfinite(pl->wf[k][(size_t)j])) return "a breakpoint or a value of a weight table is NaN or infinite";
            if (j && !(pl->wv[k][(size_t)j - 1] < pl->wv[k][(size_t)j])) return "the breakpoints of a weight table are not strictly ascending";
        }
    }
    if (c->n_x < 1 || c->n_y < 1) return "n_x and n_y must be >= 1";
    if (c->n_x + 1 > COMP_MAX_EDGES || c->n_y + 1 > COMP_MAX_EDGES) return "n_x + 1 and n_y + 1 must be at most 1024";
    if (!c->edges_x || !c->edges_y) return "edges_x or edges_y is NULL";
    if (c->plane == CPOL_COMP_PLANE_GATES) {
        if (!c->gate_x || !c->gate_y) return "gate_x or gate_y is NULL";
    } else if (!c->ray_sin || !c->ray_cos) return "ray_sin or ray_cos is NULL";
    pl->n_x = c->n_x; pl->n_y = c->n_y;
    pl->cells = (long)c->n_x * c->n_y;
    pl->block_cells = (long)(c->n_z > 0 ? c->n_z : 1) * pl->cells;
    if (c->rays_per_block < 0 || (c->rays_per_block > 0 && call.n_rows % c->rays_per_block != 0))
        return "rays_per_block must be >= 0 and divide the rows of the call";
    pl->rows_per_block = c->rays_per_block ? c->rays_per_block : call.n_rows;
    pl->n_blocks = call.n_rows / pl->rows_per_block;
    // the state (n_blocks <= 2^31 rows, cells < 2^20, at most 9 * 28 bytes per cell and block, or 64 layers of 9 * 16 bytes: no
    // overflow of long)
    const long per = pl->n_blocks * pl->block_cells;
    // (the exact sums: 260 bytes per cell and block -- beyond the limit before the product below could overflow)
    if (pl->sum && per > COMP_MAX_STATE_BYTES / COMP_SUM_ROW_BYTES) return "the state of all blocks and fields must be at most 1 GiB";
    for (int k = 0; k < COMP_FIELDS; ++k) pl->off_sum[k] = pl->off_skip[k] = -1;
    long off = 0;
    for (int i = 0; i < pl->n_fields; ++i) {
        const int k = pl->field[i];
        pl->off_max[k] = pl->off_top[k] = pl->off_low[k] = -1;
        if (c->products & CPOL_COMP_MAX) { pl->off_max[k] = off; off += per * 8; }
        pl->off_count[k] = off; off += per * 8;
        if (pl->n_thr[k]) { pl->off_top[k] = off; off += (per * pl->n_thr[k] * 4 + 7) & ~7L; }
        if (pl->sum) {
            pl->off_sum[k] = off; off += per * COMP_SUM_ROW_BYTES;
            pl->off_skip[k] = off; off += (per * 4 + 7) & ~7L;
        }
        if (off > COMP_MAX_STATE_BYTES) return "the state of all blocks and fields must be at most 1 GiB";
    }
    pl->zero_bytes = off;
    if (c->products & CPOL_COMP_LOWEST)
        for (int i = 0; i < pl->n_fields; ++i) { pl->off_low[pl->field[i]] = off; off += per * 8; }
    if (off > COMP_MAX_STATE_BYTES) return "the state of all blocks and fields must be at most 1 GiB";
    pl->state_bytes = off;
    for (int k = 0; k < COMP_FIELDS; ++k) pl->off_src_max[k] = pl->off_src_low[k] = -1;
    if (pl->with_source) {
        for (int i = 0; i < pl->n_fields; ++i) {
            const int k = pl->field[i];
            if (c->products & CPOL_COMP_MAX) { pl->off_src_max[k] = off; off += (per + 7) & ~7L; }
            if (c->products & CPOL_COMP_LOWEST) { pl->off_src_low[k] = off; off += (per + 7) & ~7L; }
        }
        pl->off_scratch = off;
        off += pl->state_bytes;
        if (off > COMP_MAX_STATE_BYTES) return "the state of all blocks and fields must be at most 1 GiB";
    }
    pl->total_bytes = off;
    // (one workgroup per stretch of a block: the grid of one launch; out of reach while the call holds fewer than 2^31 gates)
    if (pl->n_blocks * ((pl->rows_per_block * (long)call.n_gates + COMP_STRETCH - 1) / COMP_STRETCH) >= (1L << 31))
        return "too many workgroups in one call";
    const char *why;
    if ((why = hist_round_edges(c->edges_x, c->n_x + 1, HIST_T_F64, &pl->ex))) return why;
    if ((why = hist_round_edges(c->edges_y, c->n_y + 1, HIST_T_F64, &pl->ey))) return why;
    pl->begin = (c->phase & 1) != 0;
    pl->finish = (c->phase & 2) != 0;
    if (!pl->begin) {
        if (!pass.open) return "a composing call with no pass open and no begin bit";
        if (pass.fields != c->fields || pass.products != c->products || pass.n_blocks != pl->n_blocks)
            return "fields, products or block count differ from the open pass";
        if (pass.plane != c->plane) return "the plane differs from the open pass";
        if (pass.slab != pl->slab || (pl->slab && (pass.h_lo != pl->h_lo || pass.h_hi != pl->h_hi)))
            return "the height slab differs from the open pass";
        for (int i = 0; i < pl->n_fields; ++i)
            if (pass.thr[pl->field[i]] != pl->thr[pl->field[i]]) return "thresholds differ from the open pass";
        if (pass.ex != pl->ex || pass.ey != pl->ey) return "edges differ from the open pass";
        if (pass.ez != pl->ez) return "the height layers differ from the open pass";
        if (pass.gaps != pl->gaps) return "gaps differ from the open pass";
        for (int k = 0; k < COMP_FIELDS; ++k)
            if (pass.tv[k] != pl->tv[k] || pass.tf[k] != pl->tf[k]) return "a column table differs from the open pass";
        for (int k = 0; k < COMP_FIELDS; ++k)
            if (pass.wv[k] != pl->wv[k] || pass.wf[k] != pl->wf[k]) return "a weight table differs from the open pass";
    }
    if (pl->finish) {
        if (!c->count) return "a finishing call needs count";
        for (int i = 0; i < pl->n_fields; ++i)
            if (!c->values[pl->field[i]]) return "a finishing call needs values for every requested field";
        for (int k = 0; k < COMP_FIELDS; ++k)
            if (!pl->tv[k].empty() && (!c->column[k] || !c->column_layers[k]))
                return "a finishing call needs column and column_layers for every field with a table";
        for (int i = 0; cs && i < pl->n_fields; ++i)
            if (!cs->sum[pl->field[i]] || !cs->sum_skipped[pl->field[i]]) return "a finishing call needs sum and sum_skipped for every requested field";
    }
    if (pl->sum) {
        // NO OVERFLOW (above): the gates of one block once this call is folded (a call holds fewer than 2^31 * 1024 gates)
        pl->sum_gates = (pl->begin ? 0ull : pass.sum_gates) + (unsigned long long)pl->rows_per_block * (unsigned long long)call.n_gates;
        if (pl->sum_gates > COMP_SUM_MAX_GATES) return "SUM: more than 2^32 - 1 gates would fold into one block of the pass";
    }
    return nullptr;
}

// after the call is queued: the pass as it now stands
inline void comp_advance(const cpol_composite *c, const CompPlan &pl, CompPass *pass)
{
    if (pl.begin) {
        pass->open = true;
        pass->fields = c->fields;
        pass->products = c->products;
        pass->plane = c->plane;
        pass->n_blocks = pl.n_blocks;
        pass->slab = pl.slab; pass->h_lo = pl.h_lo; pass->h_hi = pl.h_hi;
        for (int k = 0; k < COMP_FIELDS; ++k) pass->thr[k] = pl.thr[k];
        pass->ex = pl.ex;
        pass->ey = pl.ey;
        pass->ez = pl.ez;
        pass->gaps = pl.gaps;
        for (int k = 0; k < COMP_FIELDS; ++k) { pass->tv[k] = pl.tv[k]; pass->tf[k] = pl.tf[k]; }
        for (int k = 0; k < COMP_FIELDS; ++k) { pass->wv[k] = pl.wv[k]; pass->wf[k] = pl.wf[k]; }
    }
    pass->sum_gates = pl.sum_gates;               // (0 without SUM)
    if (pl.finish) pass->open = false;
}
