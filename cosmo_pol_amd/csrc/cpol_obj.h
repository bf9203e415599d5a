// cpol_obj.h -- object cells (cpol_objects): every refusal and every size, decided by obj_check() from plain numbers on top of
// a FracPlan that passed, and the pieces of the labelling that do not depend on how the work is cut: the runs of a 64-cell chunk
// from the ballot of its flags, find, union and the rule that says which cell unites with which cell of the row above.  Plain C++
// that compiles for the host too (tests/c_host/obj_check.cpp drives the same functions single-threaded and compares with the
// rule), so that a merge bug shows as a wrong label on the host, not as a hang on the device.  The kernels are k_obj_*
// (cpol_obj.inl); the rule is stated in include/cosmo_pol_amd.h and cosmo_pol_amd/objects.py.
//
// THE LABEL ARRAY.  L[i] of a set cell i is the flat index of a cell of the same object with L[i] <= i; L[i] == i makes i a root;
// an unset cell holds OBJ_NONE.  It starts as the first cell of the cell's row run (no atomic for horizontal connectivity).  A
// union links the larger root to the smaller one with an atomic minimum, so L[i] <= i holds at every moment, `find` walks strictly
// downward, and the root of a finished object is its smallest flat index: the rule's first cell.
// TERMINATION.  obj_find: r strictly decreases (it stops at the first L[r] >= r, whatever the array holds).  obj_union: the larger
// index of the pair strictly decreases (it stops at the first return value >= it).  Neither waits for another thread.
#pragma once

#include "cpol_frac.h"

#if defined(__HIPCC__)
#define OBJ_HD __host__ __device__ __forceinline__
#else
#define OBJ_HD inline
#endif

constexpr int OBJ_WORDS = CPOL_OBJ_WORDS;
constexpr int OBJ_MAX_OBJECTS = CPOL_OBJ_MAX_OBJECTS;
constexpr unsigned OBJ_NONE = 0xFFFFFFFFu;
constexpr long OBJ_MAX_SCRATCH_BYTES = FRAC_MAX_SCRATCH_BYTES;
constexpr int OBJ_THREADS = FRAC_THREADS;             // threads of a workgroup: four wavefronts, one row each
constexpr int OBJ_ROWS = OBJ_THREADS / 64;
// the words of a table row
enum { OBJ_FIRST, OBJ_AREA, OBJ_SUM_X, OBJ_SUM_Y, OBJ_X0, OBJ_X1, OBJ_Y0, OBJ_Y1, OBJ_PEAK_CELL, OBJ_PEAK_BITS };

// a call that passed: the numbers the launches need
struct ObjPlan {
    bool on = false, labels = false;
    int connectivity = 0, min_area = 0, max_objects = 0;
    long n_maps = 0;                                  // (n_blocks + 1) * n_thr: map (s * n_thr + t) of source s and threshold t
    long cells = 0;
    // scratch, uint32: L [n_maps][cells]; aux [n_maps][cells] (at the roots: the area, then the object's number); rowcnt [n_maps][n_y]
    // (the kept roots of a row)
    long scratch_bytes = 0;
    long grid_rows = 0, grid_cells = 0, grid_decode = 0;   // workgroups: a wavefront per (source, row); a thread per cell; per table row
    size_t n_bytes = 0, table_bytes = 0, labels_bytes = 0;
};

// every refusal of a cpol_objects beside a cpol_fractions whose plan `fp` passed; o == NULL: off (*pl says so).  NULL: accepted
// and *pl filled; else the reason (CPOL_ERR_ARG).  Touches nothing else.
inline const char *obj_check(const cpol_objects *o, const FracPlan &fp, ObjPlan *pl)
{
    *pl = ObjPlan{};
    if (!o) return nullptr;
    if (o->connectivity != 4 && o->connectivity != 8) return "connectivity must be 4 or 8";
    if (o->min_area < 1) return "min_area must be at least 1";
    if (o->max_objects < 1 || o->max_objects > OBJ_MAX_OBJECTS) return "max_objects must lie in 1 ... 65535";
    if (!o->n_objects || !o->table) return "n_objects or table is NULL";
    if ((uintptr_t)o->table & 7u) return "table must be 8-byte aligned";
    pl->on = true; pl->labels = o->labels != nullptr;
    pl->connectivity = o->connectivity; pl->min_area = o->min_area; pl->max_objects = o->max_objects;
    pl->n_maps = fp.n_tables; pl->cells = fp.cells;
    // (n_maps * cells < 2^28 under the summed-area tables' cap, which passed: no overflow of long)
    pl->scratch_bytes = pl->n_maps * (2 * pl->cells + fp.n_y) * 4;
    if (pl->scratch_bytes > OBJ_MAX_SCRATCH_BYTES) return "the labelling scratch of all blocks and thresholds must be at most 1 GiB";
    pl->grid_rows = (fp.n_blocks + 1) * ((fp.n_y + OBJ_ROWS - 1) / OBJ_ROWS);
    pl->grid_cells = (pl->n_maps * pl->cells + OBJ_THREADS - 1) / OBJ_THREADS;
    pl->grid_decode = (pl->n_maps * pl->max_objects + OBJ_THREADS - 1) / OBJ_THREADS;
    if (pl->grid_rows >= (1L << 31) || pl->grid_cells >= (1L << 31) || pl->grid_decode >= (1L << 31)) return "too many workgroups in one call";
    pl->n_bytes = (size_t)pl->n_maps * sizeof(uint32_t);
    pl->table_bytes = (size_t)pl->n_maps * pl->max_objects * OBJ_WORDS * sizeof(uint32_t);
    pl->labels_bytes = pl->labels ? (size_t)pl->n_maps * pl->cells * sizeof(int32_t) : 0;
    return nullptr;
}

// ---- the runs of a chunk of 64 cells from the ballot `m` of its flags (bit l: cell x0 + l is set) ----

// the chunk bit at which the run of the set lane `lane` begins; 0 also when the run reaches the chunk's left border
// (obj_run_open: then the carry says where it began)
OBJ_HD int obj_run_first(unsigned long long m, int lane)
{
    const unsigned long long z = ~m & ((1ull << lane) - 1ull);        // the unset cells below the lane
    return z ? 64 - __builtin_clzll(z) : 0;
}

OBJ_HD bool obj_run_open(unsigned long long m, int lane) { return (~m & ((1ull << lane) - 1ull)) == 0ull; }

// the set cells from the set lane `lane` to the end of its run inside the chunk, 1 ... 64 - lane
OBJ_HD int obj_run_len(unsigned long long m, int lane)
{
    const unsigned long long z = ~(m >> lane);                        // (the shift fills with unset cells: the run ends in the chunk)
    return z ? __builtin_ctzll(z) : 64;
}

// the carry behind a chunk that begins at x0: the x at which the run that touches the chunk's right border began, -1: none does
OBJ_HD int obj_carry(unsigned long long m, int x0, int carry)
{
    if (!(m >> 63)) return -1;
    const unsigned long long z = ~m;
    if (!z) return carry >= 0 ? carry : x0;
    return x0 + 64 - __builtin_clzll(z);
}

// ---- find and union ----

OBJ_HD unsigned obj_load(const unsigned *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // (other workgroups lower L while this one reads)
#else
    return *p;
#endif
}

OBJ_HD unsigned obj_atomic_min(unsigned *p, unsigned v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, v);
#else
    const unsigned old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

// the root of the set cell i: r strictly decreases
OBJ_HD unsigned obj_find(const unsigned *L, unsigned i)
{
    unsigned r = i;
    for (;;) {
        const unsigned up = obj_load(L + r);
        if (up >= r) return r;
        r = up;
    }
}

// unite the objects of the set cells a and b.  The pair (hi, lo) with hi > lo: L[hi] = min(L[hi], lo).  Was hi a root (the value
// returned is hi), the two are one.  Else hi hung under `old` < hi, and whichever of old and lo lost the minimum must still be
// united with the other: the pair (old, lo), whose larger member is below hi.  So hi strictly decreases.
OBJ_HD void obj_union(unsigned *L, unsigned a, unsigned b)
{
    unsigned hi = obj_find(L, a), lo = obj_find(L, b);
    while (hi != lo) {
        if (hi < lo) { const unsigned s = hi; hi = lo; lo = s; }
        const unsigned old = obj_atomic_min(L + hi, lo);
        if (old >= hi) break;
        hi = old;
    }
}

// The unions of the set or unset cell (y, x), y >= 1, with the row above: ONE union per pair of touching runs.  me, up: the flags
// of the two rows (L != OBJ_NONE).  Edges: the two runs share a column; the union is made at the first shared column.  Corners
// (connectivity 8) add the two pairs that touch diagonally alone: the run above ends at x - 1 and this one begins at x, or the run
// above begins at x + 1 and this one ends at x.
OBJ_HD void obj_merge_cell(unsigned *L, int n_x, int y, int x, int connectivity)
{
    const unsigned *const me = L + (long)y * n_x, *const up = me - n_x;
    if (me[x] == OBJ_NONE) return;
    const unsigned i = (unsigned)(y * n_x + x), j = i - (unsigned)n_x;
    const bool a0 = up[x] != OBJ_NONE, am = x > 0 && up[x - 1] != OBJ_NONE, bm = x > 0 && me[x - 1] != OBJ_NONE;
    if (a0 && !(am && bm)) obj_union(L, i, j);
    if (connectivity == 8 && !a0) {
        const bool ap = x + 1 < n_x && up[x + 1] != OBJ_NONE, bp = x + 1 < n_x && me[x + 1] != OBJ_NONE;
        if (am && !bm) obj_union(L, i, j - 1u);
        if (ap && !bp) obj_union(L, i, j + 1u);
    }
}

// ---- the peak: the value's place in the total order of float32 (-0.0 before +0.0) above the complement of the flat index, so that
// ONE unsigned 64-bit maximum picks the largest value and, among equal bits, the smallest index.  Never 0 for a cell (NaN is never
// set, so the order word of a set cell is at least that of -inf, 0x007FFFFF). ----
OBJ_HD unsigned obj_order(unsigned bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
OBJ_HD unsigned obj_unorder(unsigned k) { return (k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k; }
OBJ_HD unsigned long long obj_peak_key(unsigned bits, unsigned cell) { return ((unsigned long long)obj_order(bits) << 32) | (unsigned long long)(~cell); }
