// cpol_obj.h -- object cells (cpol_objects): every refusal and every size, decided by obj_check() from plain numbers on top of
// a FracPlan that passed, and the pieces of the labelling that do not depend on how the work is cut: the runs of a 64-cell chunk
// from the ballot of its flags, find, union and the rule that says which cell unites with which cell of the row above.  Plain C++
// that compiles for the host too (tests/c_host/obj_check.cpp drives the same functions single-threaded and compares with the
// rule), so that a merge bug shows as a wrong label on the host, not as a hang on the device.  The kernels are k_obj_*
// (cpol_obj.inl); the rule is stated in include/cosmo_pol_amd.h and cosmo_pol_amd/objects.py.  The match (cpol_objects_match)
// runs the same run, union and find code on the overlap map of two label maps: its checks, sizes and per-cell functions are
// here too (obj_check_match, obj_match_flag, obj_match_cover; tests/c_host/obj_match_check.cpp).  The track
// (cpol_objects_track) matches every block's label map, shifted, with the next block's: its checks and sizes (obj_check_track), the
// window, count and key functions of the correlation and the shifted lookup are here as well (obj_track_*;
// tests/c_host/obj_track_check.cpp).
//
// THE LABEL ARRAY.  L[i] of a set cell i is the flat index of a cell of the same object with L[i] <= i; L[i] == i makes i a root;
// an unset cell holds OBJ_NONE.  It starts as the first cell of the cell's row run (no atomic for horizontal connectivity).  A
// union links the larger root to the smaller one with an atomic minimum, so L[i] <= i holds at every moment, `find` walks strictly
// downward, and the root of a finished object is its smallest flat index: the rule's first cell.
// TERMINATION.  obj_find: r strictly decreases (it stops at the first L[r] >= r, whatever the array holds).  obj_union: the larger
// index of the pair strictly decreases (it stops at the first return value >= it).  Neither waits for another thread.
#pragma once

#include <cmath>
#include <vector>
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
// the exact sums: the bins of one accumulator row, int64 each: OBJ_SUM_VOL_BINS of the volume, then OBJ_SUM_MOM_BINS of each moment
constexpr int OBJ_SUM_VOL_BINS = 16, OBJ_SUM_MOM_BINS = 32, OBJ_SUM_BINS = OBJ_SUM_VOL_BINS + 2 * OBJ_SUM_MOM_BINS;
constexpr int OBJ_SUM_LIMBS = 6;                      // 384 bits hold every sum (obj_sum_round)
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
    // the exact sums (cpol_objects.sums): behind the labelling scratch, 8-byte aligned, the accumulators int64 [n_maps * max_objects
    // + n_sources][OBJ_SUM_BINS], cleared in the call, then the weight table (n_weight float64 values, n_weight float32 breakpoints)
    bool sums = false;
    long n_sources = 0, acc_offset = 0, acc_bytes = 0, weight_offset = 0;
    long grid_finish = 0;                             // workgroups: a thread per (table row or source, sum); k_obj_sums takes grid_rows
    size_t volume_bytes = 0, skipped_bytes = 0, field_bytes = 0, field_cells_bytes = 0;
    std::vector<float> weight_v;                      // empty: w = m
    std::vector<double> weight_f;
    // the match (cpol_objects_match): the overlap pieces of every block's label map and the observed one.  piece_maps = n_blocks *
    // n_thr: piece map (b * n_thr + t).  The piece scratch, uint32: L, aux and rowcnt as above of piece_maps maps, behind everything
    // above on an 8-byte boundary (what lies before it does not move)
    bool match = false;
    int max_pieces = 0;
    long piece_maps = 0, piece_offset = 0, piece_bytes = 0;
    long grid_piece_rows = 0, grid_piece_cells = 0, grid_piece_decode = 0;   // as grid_rows, grid_cells and grid_decode, of the piece maps
    size_t n_pieces_bytes = 0, pieces_bytes = 0, covered_bytes = 0;
    // the track (cpol_objects_track): the pieces of every block's label map, shifted, against the next block's.  track_maps =
    // (n_blocks - 1) * n_thr: piece map (p * n_thr + t).  The track scratch behind everything above on an 8-byte boundary: the
    // packed masks uint64 [n_blocks * n_thr][n_y][track_words], the piece scratch of track_maps maps, then (correlation computed
    // but not wanted) the counters uint32 [track_maps][side][side]
    bool track = false, track_corr = false, track_corr_wanted = false;   // track_corr: max_shift >= 0
    int track_shift = 0, track_side = 0, track_words = 0, track_pieces = 0, n_pairs = 0;
    long track_maps = 0, track_bits_offset = 0, track_piece_offset = 0, track_piece_bytes = 0, track_corr_offset = 0;
    long grid_track_bits = 0, grid_track_corr = 0, track_slabs = 0, grid_track_shift = 0;   // workgroups of k_track_bits, _corr, _shift
    long grid_track_rows = 0, grid_track_cells = 0, grid_track_decode = 0;                  // as grid_piece_*, of the track's piece maps
    size_t track_corr_bytes = 0, track_shift_bytes = 0, track_n_bytes = 0, track_pieces_bytes = 0, track_covered_bytes = 0;
    std::vector<int32_t> shifts_in;                   // the given shifts, checked (max_shift == -1)
};

// the two halves of obj_check: the cells with the exact sums, then the match behind them
inline const char *obj_check_cells(const cpol_objects *o, const FracPlan &fp, ObjPlan *pl);
inline const char *obj_check_match(const cpol_objects *o, const FracPlan &fp, ObjPlan *pl);
inline const char *obj_check_track(const cpol_objects *o, const FracPlan &fp, ObjPlan *pl);

// every refusal of a cpol_objects beside a cpol_fractions whose plan `fp` passed; o == NULL: off (*pl says so).  NULL: accepted
// and *pl filled; else the reason (CPOL_ERR_ARG).  Touches nothing else.  o->pad_ != 0: *o is the first member of a
// cpol_objects_match, and only then is anything behind the cpol_objects read.
inline const char *obj_check(const cpol_objects *o, const FracPlan &fp, ObjPlan *pl)
{
    *pl = ObjPlan{};
    if (!o) return nullptr;
    if (const char *why = obj_check_cells(o, fp, pl)) return why;
    if (const char *why = obj_check_match(o, fp, pl)) return why;
    return obj_check_track(o, fp, pl);
}

inline const char *obj_check_cells(const cpol_objects *o, const FracPlan &fp, ObjPlan *pl)
{
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
    // the exact sums: a zero tail of the struct means off, and nothing above changes
    if (o->sums != 0 && o->sums != 1) return "sums must be 0 or 1";
    if (!o->sums) return nullptr;
    if (!o->volume || !o->skipped || !o->field || !o->field_cells) return "volume, skipped, field or field_cells is NULL";
    if (((uintptr_t)o->volume | (uintptr_t)o->field) & 7u) return "volume and field must be 8-byte aligned";
    if (o->n_weight != 0) {
        const int n = o->n_weight;
        if (n < 2 || n > COMP_MAX_TABLE) return "a weight table needs 2 ... 1024 breakpoints";
        if (!o->weight_v || !o->weight_f) return "weight_v or weight_f is NULL";
        pl->weight_v.assign(o->weight_v, o->weight_v + n);
        pl->weight_f.assign(o->weight_f, o->weight_f + n);
        for (int j = 0; j < n; ++j) {
            if (!std::isfinite(pl->weight_v[(size_t)j]) || !std::isfinite(pl->weight_f[(size_t)j])) return "a breakpoint or a value of the weight table is NaN or infinite";
            if (j && !(pl->weight_v[(size_t)j - 1] < pl->weight_v[(size_t)j])) return "the breakpoints of the weight table are not strictly ascending";
            if (j && !(pl->weight_f[(size_t)j - 1] <= pl->weight_f[(size_t)j])) return "the values of the weight table decrease";
        }
    }
    pl->sums = true;
    pl->n_sources = fp.n_blocks + 1;
    pl->acc_offset = (pl->scratch_bytes + 7) & ~7L;
    // (n_maps <= 4 * 2^28 / cells and max_objects < 2^16: below 2^53 bytes, no overflow of long)
    pl->acc_bytes = (pl->n_maps * pl->max_objects + pl->n_sources) * OBJ_SUM_BINS * 8;
    pl->weight_offset = pl->acc_offset + pl->acc_bytes;
    pl->scratch_bytes = pl->weight_offset + (long)o->n_weight * 8 + (((long)o->n_weight * 4 + 7) & ~7L);
    if (pl->scratch_bytes > OBJ_MAX_SCRATCH_BYTES) return "the labelling scratch and the sums' accumulators must be at most 1 GiB";
    pl->grid_finish = ((pl->n_maps * pl->max_objects + pl->n_sources) * 3 + OBJ_THREADS - 1) / OBJ_THREADS;
    if (pl->grid_finish >= (1L << 31)) return "too many workgroups in one call";
    pl->volume_bytes = (size_t)pl->n_maps * pl->max_objects * 3 * sizeof(double);
    pl->skipped_bytes = (size_t)pl->n_maps * pl->max_objects * sizeof(uint32_t);
    pl->field_bytes = (size_t)pl->n_sources * 3 * sizeof(double);
    pl->field_cells_bytes = (size_t)pl->n_sources * 2 * sizeof(uint32_t);
    return nullptr;
}

inline const char *obj_check_match(const cpol_objects *o, const FracPlan &fp, ObjPlan *pl)
{
    // (bit 30, CPOL_OBJ_TRACK, announces a cpol_objects_track around the match: obj_check_track; the low bits stay max_pieces)
    const int pad = o->pad_ < 0 ? -1 : o->pad_ & ~CPOL_OBJ_TRACK;
    if (pad < 0 || pad > OBJ_MAX_OBJECTS) return "pad_ (max_pieces of a cpol_objects_match) must lie in 0 ... 65535";
    if (!pad) return nullptr;
    const cpol_objects_match *const mo = (const cpol_objects_match *)o;
    if (!mo->n_pieces || !mo->pieces || !mo->covered) return "n_pieces, pieces or covered is NULL";
    pl->match = true; pl->max_pieces = pad;
    pl->piece_maps = (long)fp.n_blocks * fp.n_thr;
    pl->piece_offset = (pl->scratch_bytes + 7) & ~7L;
    pl->piece_bytes = pl->piece_maps * (2 * pl->cells + fp.n_y) * 4;
    pl->scratch_bytes = pl->piece_offset + pl->piece_bytes;
    if (pl->scratch_bytes > OBJ_MAX_SCRATCH_BYTES) return "the labelling scratch, the sums' accumulators and the piece scratch must be at most 1 GiB";
    pl->grid_piece_rows = (long)fp.n_blocks * ((fp.n_y + OBJ_ROWS - 1) / OBJ_ROWS);
    pl->grid_piece_cells = (pl->piece_maps * pl->cells + OBJ_THREADS - 1) / OBJ_THREADS;
    pl->grid_piece_decode = (pl->piece_maps * pl->max_pieces + OBJ_THREADS - 1) / OBJ_THREADS;
    if (pl->grid_piece_rows >= (1L << 31) || pl->grid_piece_cells >= (1L << 31) || pl->grid_piece_decode >= (1L << 31)) return "too many workgroups in one call";
    pl->n_pieces_bytes = (size_t)pl->piece_maps * sizeof(uint32_t);
    pl->pieces_bytes = (size_t)pl->piece_maps * pl->max_pieces * OBJ_WORDS * sizeof(uint32_t);
    pl->covered_bytes = (size_t)pl->piece_maps * 2 * pl->max_objects * sizeof(uint32_t);
    return nullptr;
}

// ---- the track (cpol_objects_track) ----
constexpr int OBJ_TRACK_MAX_SHIFT = CPOL_TRACK_MAX_SHIFT, OBJ_TRACK_MAX_GIVEN = CPOL_TRACK_MAX_GIVEN;
constexpr int OBJ_TRACK_ROWS = 16;                    // the earlier rows one workgroup of k_track_corr takes

// every refusal of the track behind a match that passed (or is off); reads behind the cpol_objects_match only with CPOL_OBJ_TRACK
inline const char *obj_check_track(const cpol_objects *o, const FracPlan &fp, ObjPlan *pl)
{
    if (!(o->pad_ & CPOL_OBJ_TRACK)) return nullptr;  // (pad_ >= 0: obj_check_match)
    const cpol_objects_track *const tr = (const cpol_objects_track *)o;
    if (fp.n_blocks < 2) return "the track needs at least two blocks";
    if (tr->max_shift < -1 || tr->max_shift > OBJ_TRACK_MAX_SHIFT) return "max_shift must lie in -1 ... 32";
    if (tr->max_shift == -1 && !tr->shifts_in) return "max_shift == -1 needs shifts_in";
    if (tr->max_shift >= 0 && tr->shifts_in) return "shifts_in belongs to max_shift == -1";
    if (tr->max_pieces < 1 || tr->max_pieces > OBJ_MAX_OBJECTS) return "max_pieces of the track must lie in 1 ... 65535";
    if (!tr->shift || !tr->n_pieces || !tr->pieces || !tr->covered) return "shift, n_pieces, pieces or covered of the track is NULL";
    pl->n_pairs = (int)fp.n_blocks - 1;
    pl->track_maps = (long)pl->n_pairs * fp.n_thr;
    if (tr->max_shift == -1) {
        pl->shifts_in.assign(tr->shifts_in, tr->shifts_in + pl->track_maps * 2);
        for (const int32_t v : pl->shifts_in)
            if (v < -OBJ_TRACK_MAX_GIVEN || v > OBJ_TRACK_MAX_GIVEN) return "a given shift must lie in -1023 ... 1023";
    }
    pl->track_corr = tr->max_shift >= 0; pl->track_corr_wanted = pl->track_corr && tr->correlation != nullptr;
    pl->track_shift = pl->track_corr ? tr->max_shift : 0; pl->track_side = 2 * pl->track_shift + 1;
    pl->track_pieces = tr->max_pieces;
    pl->track_words = (fp.n_x + 63) / 64;
    pl->track_bits_offset = (pl->scratch_bytes + 7) & ~7L;
    pl->track_piece_offset = pl->track_bits_offset + (long)fp.n_blocks * fp.n_thr * fp.n_y * pl->track_words * 8;
    pl->track_piece_bytes = pl->track_maps * (2 * pl->cells + fp.n_y) * 4;
    pl->track_corr_offset = pl->track_piece_offset + pl->track_piece_bytes;
    pl->track_corr_bytes = pl->track_corr ? (size_t)pl->track_maps * pl->track_side * pl->track_side * sizeof(uint32_t) : 0;
    pl->scratch_bytes = pl->track_corr_offset + (pl->track_corr && !pl->track_corr_wanted ? (long)pl->track_corr_bytes : 0);
    if (pl->scratch_bytes > OBJ_MAX_SCRATCH_BYTES) return "the scratch with the track's masks and piece maps must be at most 1 GiB";
    const long row_groups = (fp.n_y + OBJ_ROWS - 1) / OBJ_ROWS;
    pl->grid_track_bits = (long)fp.n_blocks * row_groups;
    pl->track_slabs = (fp.n_y + OBJ_TRACK_ROWS - 1) / OBJ_TRACK_ROWS;
    pl->grid_track_corr = pl->track_maps * pl->track_slabs;
    pl->grid_track_shift = (pl->track_maps + OBJ_ROWS - 1) / OBJ_ROWS;
    pl->grid_track_rows = (long)pl->n_pairs * row_groups;
    pl->grid_track_cells = (pl->track_maps * pl->cells + OBJ_THREADS - 1) / OBJ_THREADS;
    pl->grid_track_decode = (pl->track_maps * pl->track_pieces + OBJ_THREADS - 1) / OBJ_THREADS;
    if (pl->grid_track_bits >= (1L << 31) || pl->grid_track_corr >= (1L << 31) || pl->grid_track_cells >= (1L << 31) ||
        pl->grid_track_decode >= (1L << 31)) return "too many workgroups in one call";
    pl->track_shift_bytes = (size_t)pl->track_maps * 2 * sizeof(int32_t);
    pl->track_n_bytes = (size_t)pl->track_maps * sizeof(uint32_t);
    pl->track_pieces_bytes = (size_t)pl->track_maps * pl->track_pieces * OBJ_WORDS * sizeof(uint32_t);
    pl->track_covered_bytes = (size_t)pl->track_maps * 2 * pl->max_objects * sizeof(uint32_t);
    pl->track = true;
    return nullptr;
}

// The 64 cells of a packed row (`words` uint64, bit l of word w: cell 64 w + l; the bits at or beyond n_x zero) from cell
// 64 w + dx on, |dx| < 64: the funnel shift of the words w and w + 1 (dx > 0) or w - 1 and w (dx < 0); cells outside the row are
// unset
OBJ_HD unsigned long long obj_track_window(const unsigned long long *row, int words, int w, int dx)
{
    const unsigned long long mid = row[w];
    if (dx == 0) return mid;
    if (dx > 0) return (mid >> dx) | (w + 1 < words ? row[w + 1] << (64 - dx) : 0ull);
    return (mid << -dx) | (w > 0 ? row[w - 1] >> (64 + dx) : 0ull);
}

// what the earlier rows [y0, y1) of a pair add to the counter (dy, dx): the cells set in Ke at (y, x) and in Kl at (y + dy, x + dx).
// A bound fixed before the loops start: (y1 - y0) * words turns
OBJ_HD unsigned obj_track_count(const unsigned long long *ke, const unsigned long long *kl, int n_y, int words, int y0, int y1, int dy, int dx)
{
    unsigned n = 0u;
    for (int y = y0; y < y1; ++y) {
        const int yl = y + dy;
        if (yl < 0 || yl >= n_y) continue;
        const unsigned long long *const e = ke + (long)y * words, *const l = kl + (long)yl * words;
        for (int w = 0; w < words; ++w) n += (unsigned)__builtin_popcountll(e[w] & obj_track_window(l, words, w, dx));
    }
    return n;
}

// The argmax of the shift as ONE unsigned 64-bit maximum: the count above the complement of (dy^2 + dx^2, dy + S, dx + S), so
// that among equal counts the smallest distance, then the smallest dy, then the smallest dx wins.  S <= 32: dy^2 + dx^2 <= 2048
// (12 bits), dy + S and dx + S <= 64 (7 bits each)
OBJ_HD unsigned long long obj_track_key(unsigned count, int dy, int dx, int S)
{
    const unsigned low = ((unsigned)(dy * dy + dx * dx) << 14) | ((unsigned)(dy + S) << 7) | (unsigned)(dx + S);
    return ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - low);
}
OBJ_HD void obj_track_unkey(unsigned long long key, int S, int *dy, int *dx)
{
    const unsigned low = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    *dy = (int)((low >> 7) & 127u) - S;
    *dx = (int)(low & 127u) - S;
}

// the kept number of the earlier block's object at cell (y, x) of the LATER frame under the shift (dy, dx): the lookup at
// (y - dy, x - dx), 0 outside the grid
OBJ_HD unsigned obj_track_number(const unsigned *L, const unsigned *aux, int n_x, int n_y, int y, int x, int dy, int dx)
{
    const int ys = y - dy, xs = x - dx;
    if (ys < 0 || ys >= n_y || xs < 0 || xs >= n_x) return 0u;
    const unsigned root = L[ys * n_x + xs];               // (obj_number_of, below)
    return root == OBJ_NONE ? 0u : aux[root];
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

// ---- the match (cpol_objects_match): the per-cell logic of k_match_runs.  After the object phase L is flattened (L[cell] = the
// root) and aux[root] = the kept number or 0. ----

OBJ_HD unsigned obj_atomic_add(unsigned *p, unsigned v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const unsigned old = *p;
    *p = old + v;
    return old;
#endif
}

// the kept number of the cell in the label map (L, aux), 0 for background and dropped objects: what `labels` would hold
OBJ_HD unsigned obj_number_of(const unsigned *L, const unsigned *aux, unsigned cell)
{
    const unsigned root = L[cell];
    return root == OBJ_NONE ? 0u : aux[root];
}

// the overlap flag of a cell from the two (root, number) lookups: *nf its number in the block's map, *no in the observed one
OBJ_HD bool obj_match_flag(const unsigned *Lf, const unsigned *auxf, const unsigned *Lo, const unsigned *auxo, unsigned cell, unsigned *nf, unsigned *no)
{
    *nf = obj_number_of(Lf, auxf, cell);
    *no = obj_number_of(Lo, auxo, cell);
    return *nf != 0u && *no != 0u;
}

// what the lane at which a run of I begins in a chunk adds for its segment of `len` cells: a run of I lies inside one run of each
// map, so nf and no are constant over it.  covered: [2][max_objects] of the (block, threshold); numbers beyond max_objects have no entry
OBJ_HD void obj_match_cover(unsigned *covered, int max_objects, unsigned nf, unsigned no, unsigned len)
{
    if (nf <= (unsigned)max_objects) obj_atomic_add(covered + (nf - 1u), len);
    if (no <= (unsigned)max_objects) obj_atomic_add(covered + max_objects + (no - 1u), len);
}

// ---- the peak: the value's place in the total order of float32 (-0.0 before +0.0) above the complement of the flat index, so that
// ONE unsigned 64-bit maximum picks the largest value and, among equal bits, the smallest index.  Never 0 for a cell (NaN is never
// set, so the order word of a set cell is at least that of -inf, 0x007FFFFF). ----
OBJ_HD unsigned obj_order(unsigned bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
OBJ_HD unsigned obj_unorder(unsigned k) { return (k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k; }
OBJ_HD unsigned long long obj_peak_key(unsigned bits, unsigned cell) { return ((unsigned long long)obj_order(bits) << 32) | (unsigned long long)(~cell); }

// ---- the exact sums (cpol_objects.sums).  A finite float32 with the bits (sign, e, m) is  +-M * 2^(E - 150)  with E = max(e, 1) in
// 1 ... 254 and M = m | (e ? 2^23 : 0) < 2^24: an INTEGER multiple of 2^-150 (of 2^-149 in fact).  Integer additions commute, so
// atomics in any order leave the same accumulator, and ONE rounding at the end gives the float64 that no order can change.
// THE ACCUMULATOR ROW, OBJ_SUM_BINS signed 64-bit bins (two's complement, added as unsigned long long):
//   volume    bins 0 ... 15:  bin E >> 4 takes  +-M << (E & 15), below 2^39 in magnitude.  An object (and the field) has < 2^20 cells
//             (NO OVERFLOW, cosmo_pol_amd.h), so |bin| < 2^59.
//   moment_x  bins 16 ... 47: bin E >> 3 takes  +-(M * ix) << (E & 7).  The sum of ix over the cells is < 2^30 (the same clause), so
//             |bin| < 2^24 * 2^7 * 2^30 = 2^61.
//   moment_y  bins 48 ... 79: likewise with iy.
// Conditions, not measurements: no bin can wrap.  The sum is  2^-150 * sum_b bin[b] * 2^(step * b)  with step 16 or 8: below 2^(8 *
// 31 + 62) = 2^310 in magnitude, which the OBJ_SUM_LIMBS * 64 = 384 bits of obj_sum_round hold with their sign. ----

// false: the value is +-inf or NaN and is not summed
OBJ_HD bool obj_sum_split(unsigned bits, int *E, unsigned *M)
{
    const unsigned e = (bits >> 23) & 0xFFu, m = bits & 0x007FFFFFu;
    *E = e ? (int)e : 1;
    *M = e ? m | 0x00800000u : m;
    return e != 0xFFu;
}

// the signed contribution  +-(M * mult) << shift  (mult <= 1023, shift <= 15 with mult 1 and <= 7 else: below 2^41)
OBJ_HD long long obj_sum_term(unsigned bits, unsigned M, unsigned mult, int shift)
{
    const long long c = (long long)(((unsigned long long)M * mult) << shift);
    return (bits & 0x80000000u) ? -c : c;
}

// The bits of the float64 nearest to  2^-150 * sum_b bins[b] * 2^(step * b)  (ties to even), +0.0 for an exact zero: the bins
// propagated into one two's-complement integer of OBJ_SUM_LIMBS limbs, its sign and magnitude, the top 53 bits, then the guard bit
// and the sticky rest.  The magnitude is >= 1 and < 2^310, so the result is a normal number: no underflow, no overflow.
OBJ_HD unsigned long long obj_sum_round(const unsigned long long *bins, int n_bins, int step)
{
    unsigned long long limb[OBJ_SUM_LIMBS];
    for (int k = 0; k < OBJ_SUM_LIMBS; ++k) limb[k] = 0ull;
    for (int b = 0; b < n_bins; ++b) {
        const unsigned long long v = bins[b], ext = (v >> 63) ? ~0ull : 0ull;
        const int w = (b * step) >> 6, s = (b * step) & 63;
        const unsigned long long lo = v << s, mid = s ? (v >> (64 - s)) | (ext << s) : ext;
        unsigned long long carry = 0ull;
        for (int k = w; k < OBJ_SUM_LIMBS; ++k) {
            const unsigned long long piece = k == w ? lo : k == w + 1 ? mid : ext;
            const unsigned long long a = limb[k] + piece, c = a + carry;
            carry = (unsigned long long)(a < piece) | (unsigned long long)(c < carry);
            limb[k] = c;
        }
    }
    const bool neg = (limb[OBJ_SUM_LIMBS - 1] >> 63) != 0ull;
    if (neg) {
        unsigned long long carry = 1ull;
        for (int k = 0; k < OBJ_SUM_LIMBS; ++k) {
            const unsigned long long c = ~limb[k] + carry;
            carry = (unsigned long long)(c < carry);
            limb[k] = c;
        }
    }
    int top = -1;
    for (int k = 0; k < OBJ_SUM_LIMBS; ++k)
        if (limb[k]) top = k;
    if (top < 0) return 0ull;
    const int p = 64 * top + 63 - __builtin_clzll(limb[top]);         // the highest set bit
    unsigned long long mant;
    if (p <= 52) mant = limb[0] << (52 - p);                          // (exact: nothing to round)
    else {
        const int r = p - 52, i = r >> 6, s = r & 63;                 // the 53 bits from bit r on
        mant = limb[i] >> s;
        if (s && i + 1 < OBJ_SUM_LIMBS) mant |= limb[i + 1] << (64 - s);
        mant &= (1ull << 53) - 1ull;
        const int g = r - 1, gi = g >> 6, gs = g & 63;
        const bool guard = (limb[gi] >> gs) & 1ull;
        bool sticky = (limb[gi] & ((1ull << gs) - 1ull)) != 0ull;
        for (int k = 0; k < gi; ++k) sticky = sticky || limb[k] != 0ull;
        if (guard && (sticky || (mant & 1ull))) ++mant;               // (2^53: the sum below carries it into the exponent)
    }
    return ((unsigned long long)neg << 63) | ((((unsigned long long)(p - 150 + 1023)) << 52) + (mant - (1ull << 52)));
}

// The weight of a cell: w = float32(f(v)), f the piecewise-linear function of composite.column_of (k_comp_column) over the table
// (tv float32 strictly ascending, tf float64) of n breakpoints, statement by statement: j = #{ tv <= v } - 1 from comparisons in
// float32 (step0: the largest power of two <= n); 0 below the table, tf[n - 1] at and above its end; else t, d, p and tf[j] + p,
// one float64 operation each (no contraction); then ONE rounding to float32.  v is not NaN.
OBJ_HD float obj_weight(const float *tv, const double *tf, int n, int step0, float v)
{
    int lo = 0;
    for (int step = step0; step > 0; step >>= 1) {
        const int t = lo + step;
        if (t <= n && tv[t - 1] <= v) lo = t;
    }
    const int j = lo - 1;
    double f;
    if (j < 0) f = 0.0;
    else if (j >= n - 1) f = tf[n - 1];
    else {
        const double t = ((double)v - (double)tv[j]) / ((double)tv[j + 1] - (double)tv[j]);
        const double d = tf[j + 1] - tf[j];
        const double p = t * d;
        f = tf[j] + p;
    }
    return (float)f;
}
