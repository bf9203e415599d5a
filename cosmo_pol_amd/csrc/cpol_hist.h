// cpol_hist.h -- sweep histograms (cpol_histogram): every refusal, the rounding of the edges to the field's type and the cell
// and block arithmetic of a call, decided by hist_check() from plain numbers.  Plain C++ without HIP types, so that a host
// program can include it (tests/c_host/hist_check.cpp, tests/test_histogram_cpu.py check it without a GPU).  The kernel is
// k_hist (cpol_hist.inl); the rule is stated in include/cosmo_pol_amd.h and cosmo_pol_amd/histogram.py.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/cosmo_pol_amd.h"

constexpr int HIST_FIELDS = CPOL_HIST_FIELDS;
constexpr int HIST_RVEL = 9;                       // the one float64 field
constexpr int HIST_MAX_EDGES = 1024;               // n + 1 of either axis
constexpr int HIST_MAX_CELLS = 16384;              // (n_x + 2) * (n_y + 2) of one field: 64 KiB of LDS as uint32
constexpr long HIST_MAX_STATE_CELLS = 1L << 27;    // n_blocks * the cells of all requested fields: 1 GiB of uint64 state
// gates per workgroup of k_hist.  Far below 2^32, so that a workgroup's uint32 cell cannot overflow; the 180 000 gates of a
// 360 x 500 sweep give 352 workgroups per field
constexpr int HIST_STRETCH = 512;
constexpr int HIST_THREADS = 256;                  // threads of a workgroup of k_hist
enum { HIST_ORD_NONE = 0, HIST_ORD_HEIGHTS = 1, HIST_ORD_DIST = 2, HIST_ORD_FIELD = 16, HIST_ORD_MODEL = 32 };
enum { HIST_T_NONE = 0, HIST_T_F32 = 1, HIST_T_F64 = 2 };

// what the entry point knows of the call
struct HistCall {
    long n_rows = 0;               // n_rays, or n_members * n_rays
    int n_gates = 0;
    bool doppler = false;          // RVEL is produced
    int n_model_vars = 0;          // rows of model_vars the call produces (0: none)
};

// the open pass of a context (the counts themselves live on the device)
struct HistPass {
    bool open = false;
    uint32_t fields = 0;
    int ordinate = 0;
    long n_blocks = 0;
    std::vector<double> ex[HIST_FIELDS], ey;       // the ROUNDED edges (widened again: exact)
};

// a call that passed: the numbers the launch needs
struct HistPlan {
    int n_fields = 0;
    int field[HIST_FIELDS] = {};                   // the requested fields, ascending
    int n_ex[HIST_FIELDS] = {};                    // edges of field k's abscissa (n_x + 1)
    int cells[HIST_FIELDS] = {};                   // (n_x + 2) * (n_y + 2)
    long state_off[HIST_FIELDS] = {};              // field k's table [n_blocks][cells] in the state, in cells
    int n_ey = 0, ny2 = 1;                         // edges of the ordinate; n_y + 2 (1: no ordinate)
    int ord_type = HIST_T_NONE;
    long n_blocks = 1, rows_per_block = 0;
    long state_cells = 0;                          // n_blocks * sum of cells
    std::vector<double> ex[HIST_FIELDS], ey;       // rounded
    bool begin = false, finish = false;
};

inline int hist_field_type(int k) { return k == HIST_RVEL ? HIST_T_F64 : HIST_T_F32; }

// the edges rounded once to the axis' type; NULL: fine; else why not
inline const char *hist_round_edges(const double *e, int n_edges, int type, std::vector<double> *out)
{
    out->resize((size_t)n_edges);
    for (int j = 0; j < n_edges; ++j) {
        const double v = e[j];
        if (!(v == v) || std::isinf(v)) return "an edge is NaN or infinite";
        // (at or beyond the midpoint between FLT_MAX and 2^128 the rounding gives infinity)
        if (type == HIST_T_F32 && std::fabs(v) >= 0x1.ffffffp+127) return "an edge is infinite after rounding to float32";
        const double r = type == HIST_T_F32 ? (double)(float)v : v;
        if (j > 0 && !(r > (*out)[(size_t)j - 1])) return "edges not strictly ascending after rounding to the field's type";
        (*out)[(size_t)j] = r;
    }
    return nullptr;
}

// every refusal of a cpol_histogram for a call; NULL: accepted and *pl filled; else the reason (CPOL_ERR_ARG).  Touches neither
// the pass nor anything else: the caller opens / closes the pass once the call is queued.
inline const char *hist_check(const cpol_histogram *h, const HistCall &c, const HistPass &pass, HistPlan *pl)
{
    *pl = HistPlan{};
    if (h->phase < 0 || h->phase > 3) return "phase must lie in 0 ... 3";
    if (h->fields == 0 || (h->fields >> HIST_FIELDS) != 0) return "fields must name at least one of the 10 fields and no other bit";
    if (((h->fields >> HIST_RVEL) & 1u) && !c.doppler) return "RVEL needs simulate_doppler";
    const int ord = h->ordinate;
    if (ord == HIST_ORD_NONE) {
        if (h->n_y != 0) return "n_y must be 0 without an ordinate";
    } else {
        if (ord == HIST_ORD_HEIGHTS || ord == HIST_ORD_DIST) pl->ord_type = HIST_T_F32;
        else if (ord >= HIST_ORD_FIELD && ord < HIST_ORD_FIELD + HIST_FIELDS) {
            if (ord - HIST_ORD_FIELD == HIST_RVEL && !c.doppler) return "RVEL as ordinate needs simulate_doppler";
            pl->ord_type = hist_field_type(ord - HIST_ORD_FIELD);
        } else if (ord >= HIST_ORD_MODEL && ord < HIST_ORD_MODEL + CPOL_MAX_VARS) {
            if (c.n_model_vars < 1) return "a model variable as ordinate needs a call that produces model_vars";
            if (ord - HIST_ORD_MODEL >= c.n_model_vars) return "the ordinate's model variable lies beyond n_vars";
            pl->ord_type = HIST_T_F64;
        } else return "unknown ordinate code";
        if (h->n_y < 1 || !h->edges_y) return "an ordinate needs n_y >= 1 and edges_y";
        if (h->n_y + 1 > HIST_MAX_EDGES) return "n_y + 1 must be at most 1024";
        pl->n_ey = h->n_y + 1;
        pl->ny2 = h->n_y + 2;
    }
    long sum = 0;
    for (int k = 0; k < HIST_FIELDS; ++k) {
        if (!((h->fields >> k) & 1u)) continue;
        if (h->n_x[k] < 1) return "n_x of a requested field must be >= 1";
        if (h->n_x[k] + 1 > HIST_MAX_EDGES) return "n_x + 1 of a requested field must be at most 1024";
        if (!h->edges_x[k]) return "edges_x of a requested field is NULL";
        const long cells = (long)(h->n_x[k] + 2) * pl->ny2;
        if (cells > HIST_MAX_CELLS) return "(n_x + 2) * (n_y + 2) of a requested field must be at most 16384 cells";
        pl->field[pl->n_fields++] = k;
        pl->n_ex[k] = h->n_x[k] + 1;
        pl->cells[k] = (int)cells;
        sum += cells;
    }
    if (h->rays_per_block < 0 || (h->rays_per_block > 0 && c.n_rows % h->rays_per_block != 0))
        return "rays_per_block must be >= 0 and divide the rows of the call";
    pl->rows_per_block = h->rays_per_block ? h->rays_per_block : c.n_rows;
    pl->n_blocks = c.n_rows / pl->rows_per_block;
    if (pl->n_blocks * sum > HIST_MAX_STATE_CELLS) return "n_blocks * the cells of the requested fields must be at most 2^27";
    // (one workgroup per stretch of a block: the grid of one launch; out of reach while the call holds fewer than 2^31 gates)
    if (pl->n_blocks * ((pl->rows_per_block * (long)c.n_gates + HIST_STRETCH - 1) / HIST_STRETCH) >= (1L << 31))
        return "too many workgroups in one call";
    pl->state_cells = pl->n_blocks * sum;
    long off = 0;
    for (int i = 0; i < pl->n_fields; ++i) {
        const int k = pl->field[i];
        pl->state_off[k] = off;
        off += pl->n_blocks * pl->cells[k];
    }
    const char *why;
    for (int i = 0; i < pl->n_fields; ++i) {
        const int k = pl->field[i];
        if ((why = hist_round_edges(h->edges_x[k], pl->n_ex[k], hist_field_type(k), &pl->ex[k]))) return why;
    }
    if (ord != HIST_ORD_NONE && (why = hist_round_edges(h->edges_y, pl->n_ey, pl->ord_type, &pl->ey))) return why;
    pl->begin = (h->phase & 1) != 0;
    pl->finish = (h->phase & 2) != 0;
    if (!pl->begin) {
        if (!pass.open) return "a counting call with no pass open and no begin bit";
        if (pass.fields != h->fields || pass.ordinate != ord || pass.n_blocks != pl->n_blocks)
            return "fields, ordinate or block count differ from the open pass";
        for (int i = 0; i < pl->n_fields; ++i)
            if (pass.ex[pl->field[i]] != pl->ex[pl->field[i]]) return "edges differ from the open pass";
        if (pass.ey != pl->ey) return "ordinate edges differ from the open pass";
    }
    if (pl->finish)
        for (int i = 0; i < pl->n_fields; ++i)
            if (!h->counts[pl->field[i]]) return "a finishing call needs counts for every requested field";
    return nullptr;
}

// after the call is queued: the pass as it now stands
inline void hist_advance(const cpol_histogram *h, const HistPlan &pl, HistPass *pass)
{
    if (pl.begin) {
        pass->open = true;
        pass->fields = h->fields;
        pass->ordinate = h->ordinate;
        pass->n_blocks = pl.n_blocks;
        for (int k = 0; k < HIST_FIELDS; ++k) pass->ex[k] = pl.ex[k];
        pass->ey = pl.ey;
    }
    if (pl.finish) pass->open = false;
}
