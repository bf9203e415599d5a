// cpol_frac.h -- neighbourhood verification (cpol_fractions): every refusal, the rounding of the thresholds to float32, where the
// scored plane lies in the composite's `values`, the layout of the summed-area tables and the grids of the three launches,
// decided by frac_check() from plain numbers.  Plain C++ without HIP types, so that a host program can include it
// (tests/c_host/frac_check.cpp, tests/test_neighbourhood_cpu.py check it without a GPU).  The kernels are k_frac_rows,
// k_frac_cols and k_frac_score (cpol_frac.inl); the rule is stated in include/cosmo_pol_amd.h and
// cosmo_pol_amd/neighbourhood.py.  The neighbourhood ensemble probabilities (cpol_fraction_probabilities, k_frac_members in
// cpol_frac_prob.inl) have their sub-plan and their refusals here too: frac_prob_check (tests/c_host/frac_prob_check.cpp,
// tests/test_neighbourhood_prob_cpu.py).
#pragma once

#include "cpol_comp.h"

constexpr int FRAC_MAX_THR = CPOL_FRAC_MAX_THRESHOLDS;
constexpr int FRAC_MAX_RADII = CPOL_FRAC_MAX_RADII;
constexpr int FRAC_MAX_RADIUS = CPOL_FRAC_MAX_RADIUS;
constexpr int FRAC_MAX_SIDE = COMP_MAX_EDGES - 1;     // cells per axis: the composite's limit
// the summed-area tables of all blocks and thresholds plus the observation's: the composite's cap for the sum of both
constexpr long FRAC_MAX_SCRATCH_BYTES = COMP_MAX_STATE_BYTES;
constexpr int FRAC_THREADS = 256;                     // threads of a workgroup of the three kernels: four wavefronts
constexpr int FRAC_ROWS = FRAC_THREADS / 64;          // rows of a workgroup of k_frac_rows: one per wavefront
// cells of a workgroup of k_frac_score, four per thread: a 300 x 300 map gives 88 workgroups per (block, threshold), each with
// ONE atomic addition per sum
constexpr int FRAC_CELLS = 4 * FRAC_THREADS;
constexpr int FRAC_PROB_MAX_BLOCKS = CPOL_FRAC_PROB_MAX_BLOCKS;   // bounds `reliability` and the LDS table of k_frac_members

// a cpol_fractions that is the first member of a cpol_fractions_ensemble says so in n_radii (a positive count or-ed with
// CPOL_FRAC_ENSEMBLE; a negative n_radii has the bit set too and is no flag): only then is anything behind the struct read
inline bool frac_is_ensemble(const cpol_fractions *f) { return f->n_radii > 0 && (f->n_radii & CPOL_FRAC_ENSEMBLE) != 0; }
inline int frac_n_radii(const cpol_fractions *f) { return frac_is_ensemble(f) ? f->n_radii & ~CPOL_FRAC_ENSEMBLE : f->n_radii; }
inline const cpol_fraction_probabilities *frac_probabilities(const cpol_fractions *f)
{
    return frac_is_ensemble(f) ? ((const cpol_fractions_ensemble *)f)->probabilities : nullptr;
}

// the neighbourhood ensemble probabilities of a call that passed (cpol_fractions_ensemble.probabilities; on == false: off)
struct FracProbPlan {
    bool on = false, member_sum = false, member_any = false;
    long grid = 0;                                    // workgroups of k_frac_members: n_thr * n_radii * score_groups
    int table_entries = 0;                            // uint32 entries of its LDS table: (n_blocks + 1) * 2
    size_t prob_sums_bytes = 0, reliability_bytes = 0, member_sum_bytes = 0, member_any_bytes = 0;
};

// a call that passed: the numbers the launches need
struct FracPlan {
    int n_thr = 0, n_radii = 0;
    float thr[FRAC_MAX_THR] = {};                     // the ROUNDED thresholds
    int radii[FRAC_MAX_RADII] = {};
    int n_x = 0, n_y = 0;
    long cells = 0, n_blocks = 0;
    // one summed-area table: uint32 [n_y + 1][n_x + 1], row 0 and column 0 zero, so that a clipped window is four look-ups with no
    // branch.  Table (s * n_thr + t) belongs to source s and threshold t; sources 0 ... n_blocks - 1 are the blocks of the plane,
    // source n_blocks is the observation: built once, read by every block
    long table = 0, n_tables = 0, scratch_bytes = 0;
    int field = 0;                                    // (sweep calls) the field whose `values` hold the plane ...
    long plane_first = 0, plane_stride = 0;           // ... block b's plane begins plane_first + b * plane_stride floats into it
    long grid_rows = 0, grid_cols = 0, grid_score = 0;   // workgroups of the three launches
    int col_chunks = 0, score_groups = 0;             // 64-column chunks of a table; workgroups of k_frac_score per (block, threshold)
    size_t sums_bytes = 0, totals_bytes = 0;
    FracProbPlan prob;
};

// NO OVERFLOW of the ensemble sums (cosmo_pol_amd.h, cpol_fraction_probabilities): with c = min(2 r_max + 1, n_y) * min(2 r_max
// + 1, n_x) the call passes only if M * c < 2^32 and n_y * n_x * (M * c)^2 < 2^64.  M * c < 2^8 * 2^20 and cells < 2^20 under
// the limits that passed, so the product is < 2^76: formed in 128 bits, the check cannot overflow itself.
inline bool frac_prob_overflows(int n_x, int n_y, long n_blocks, int r_max)
{
    const long side = 2L * r_max + 1;
    const unsigned __int128 c = (unsigned __int128)(side < n_y ? side : n_y) * (unsigned __int128)(side < n_x ? side : n_x);
    const unsigned __int128 mc = (unsigned __int128)n_blocks * c;
    if (mc >> 32) return true;
    return (((unsigned __int128)n_y * (unsigned __int128)n_x * mc * mc) >> 64) != 0;
}

// every refusal of a cpol_fraction_probabilities beside a cpol_fractions whose plan *pl passed so far; q == NULL: off.  NULL:
// accepted and pl->prob filled; else the reason (CPOL_ERR_ARG).  Touches nothing else.
inline const char *frac_prob_check(const cpol_fraction_probabilities *q, FracPlan *pl)
{
    pl->prob = FracProbPlan{};
    if (!q) return nullptr;
    if (!q->prob_sums || !q->reliability) return "probabilities: prob_sums or reliability is NULL";
    if (pl->n_blocks > FRAC_PROB_MAX_BLOCKS) return "probabilities: at most 256 blocks (CPOL_FRAC_PROB_MAX_BLOCKS)";
    if (frac_prob_overflows(pl->n_x, pl->n_y, pl->n_blocks, pl->radii[pl->n_radii - 1]))
        return "probabilities: the sums could overflow (needs n_blocks * c < 2^32 and n_y * n_x * (n_blocks * c)^2 < 2^64, c the cells of the largest clipped window)";
    FracProbPlan &pp = pl->prob;
    pp.on = true; pp.member_sum = q->member_sum != nullptr; pp.member_any = q->member_any != nullptr;
    pp.grid = (long)pl->n_thr * pl->n_radii * pl->score_groups;       // (at most 4 * 8 * 1022 workgroups)
    pp.table_entries = ((int)pl->n_blocks + 1) * 2;
    pp.prob_sums_bytes = (size_t)pl->n_thr * pl->n_radii * 3 * sizeof(uint64_t);
    pp.reliability_bytes = (size_t)pl->n_thr * pl->n_radii * pp.table_entries * sizeof(uint64_t);
    const size_t map_bytes = (size_t)pl->n_thr * pl->n_radii * (size_t)pl->cells * sizeof(uint32_t);
    pp.member_sum_bytes = pp.member_sum ? map_bytes : 0;
    pp.member_any_bytes = pp.member_any ? map_bytes : 0;
    return nullptr;
}

// what does not depend on the composite: thresholds, radii, pointers, the scratch and the grids for n_blocks maps of n_y x n_x
inline const char *frac_check_maps(const cpol_fractions *f, int n_x, int n_y, long n_blocks, FracPlan *pl)
{
    if (n_x < 1 || n_y < 1 || n_x > FRAC_MAX_SIDE || n_y > FRAC_MAX_SIDE || n_blocks < 1) return "the maps need 1 ... 1023 cells per axis and at least one block";
    if (f->n_thresholds < 1 || f->n_thresholds > FRAC_MAX_THR) return "n_thresholds must lie in 1 ... 4";
    for (int j = 0; j < f->n_thresholds; ++j) {
        const double t = f->thresholds[j];
        if (!(t == t)) return "a threshold is NaN";
        pl->thr[j] = comp_f32(t);
    }
    const int n_radii = frac_n_radii(f);
    if (n_radii < 1 || n_radii > FRAC_MAX_RADII) return "n_radii must lie in 1 ... 8";
    for (int j = 0; j < n_radii; ++j) {
        if (f->radii[j] < 0 || f->radii[j] > FRAC_MAX_RADIUS) return "a radius must lie in 0 ... 1023";
        if (j > 0 && f->radii[j] <= f->radii[j - 1]) return "the radii must be strictly ascending";
        pl->radii[j] = f->radii[j];
    }
    if (!f->observed) return "observed is NULL";
    if (!f->sums || !f->totals) return "sums or totals is NULL";
    pl->n_thr = f->n_thresholds; pl->n_radii = n_radii;
    pl->n_x = n_x; pl->n_y = n_y; pl->cells = (long)n_x * n_y; pl->n_blocks = n_blocks;
    pl->table = (long)(n_y + 1) * (n_x + 1);
    // (n_blocks < 2^31 rows of a call, at most 4 thresholds and 2^20 entries of 4 bytes: no overflow of long)
    pl->n_tables = (n_blocks + 1) * pl->n_thr;
    pl->scratch_bytes = pl->n_tables * pl->table * 4;
    if (pl->scratch_bytes > FRAC_MAX_SCRATCH_BYTES) return "the summed-area tables of all blocks and thresholds must be at most 1 GiB";
    pl->col_chunks = (n_x + 63) / 64;
    pl->score_groups = (int)((pl->cells + FRAC_CELLS - 1) / FRAC_CELLS);
    pl->grid_rows = (n_blocks + 1) * ((n_y + FRAC_ROWS - 1) / FRAC_ROWS);
    pl->grid_cols = pl->n_tables * pl->col_chunks;
    pl->grid_score = n_blocks * pl->n_thr * pl->score_groups;
    // (each launch has fewer workgroups than the tables have entries, 2^28 under the cap: out of reach, stated for the reader)
    if (pl->grid_rows >= (1L << 31) || pl->grid_cols >= (1L << 31) || pl->grid_score >= (1L << 31)) return "too many workgroups in one call";
    pl->sums_bytes = (size_t)n_blocks * pl->n_thr * pl->n_radii * 3 * sizeof(uint64_t);
    pl->totals_bytes = (size_t)n_blocks * pl->n_thr * 3 * sizeof(uint64_t);
    return frac_prob_check(frac_probabilities(f), pl);
}

// every refusal of a cpol_fractions for a sweep call; c: the call's cpol_composite (NULL: none), cp: its plan, which passed
// comp_check.  NULL: accepted and *pl filled; else the reason (CPOL_ERR_ARG).  Touches nothing else.
inline const char *frac_check(const cpol_fractions *f, const cpol_composite *c, const CompPlan *cp, FracPlan *pl)
{
    *pl = FracPlan{};
    if (!c || !cp) return "needs a composite (outputs->composite) in the same call";
    if (cp->n_z > 0) return "a composite with height layers is not scored (the planes carry a layer axis; the column is no plane)";
    if (!cp->finish) return "the composite call does not finish its pass (phase & 2): the maps do not exist yet";
    if (f->field < 0 || f->field >= COMP_FIELDS || !((c->fields >> f->field) & 1u)) return "field is not among the composed fields (composite->fields)";
    const int n_planes = cp->n_planes[f->field];
    if (f->plane < 0 || f->plane >= n_planes) return "plane lies outside the planes of the field";
    const char *why = frac_check_maps(f, cp->n_x, cp->n_y, cp->n_blocks, pl);
    if (why) return why;
    pl->field = f->field;
    pl->plane_first = (long)f->plane * pl->cells;
    pl->plane_stride = (long)n_planes * pl->cells;
    return nullptr;
}
