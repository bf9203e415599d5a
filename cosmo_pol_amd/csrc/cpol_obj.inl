// cpol_obj.inl -- object cells: the connected components of the binary maps of a neighbourhood verification, numbered in raster
// order of their first cells, with ten integer attributes each (cpol_objects).
//
// Reference functions replaced (wolfidan/cosmo_pol): none -- a verification group pulls every map to the host and labels it there.
// The rule is the one of include/cosmo_pol_amd.h and cosmo_pol_amd/objects.py (`cells`).  Every number is an integer or a
// comparison, so the result is the rule's whatever order the hardware works in.  The labelling is a label-equivalence union-find
// (cpol_obj.h): L[i] <= i always, a union is an atomic minimum.  NO kernel waits on another workgroup -- no spin, no flag, no
// grid-wide barrier: what must be complete before the next step is complete because the launch before it has ended -- and every
// loop carries a strictly decreasing unsigned integer (cpol_obj.h, TERMINATION), or counts up to a bound fixed before it starts.
//
// Eight launches behind k_frac_score; a wavefront owns one row of one source and handles all thresholds, as in k_frac_rows:
//   k_obj_runs     the binary maps again from ONE read of the row; L = the first cell of the cell's row run, from the ballot;
//   k_obj_merge    one union per pair of touching runs of a row and the row above (obj_merge_cell);
//   k_obj_flatten  a thread per cell: L = find(L); the areas cleared;
//   k_obj_area     one integer addition per run segment at its root;
//   k_obj_count    the kept roots (root && area >= min_area) of every row;
//   k_obj_number   the kept roots numbered: the rows above summed, the ballot prefix inside the row; n_objects; first and area
//                  into the table; the root's area gives way to its number;
//   k_obj_attr     the labels, and per run segment the sums, the box and the peak into the table rows up to max_objects;
//   k_obj_decode   a thread per table row: the box and the peak out of the forms the atomic maxima needed.
// With cpol_objects.sums two more (the EXACT SUMS of the header; the accumulator row and its bounds: cpol_obj.h):
//   k_obj_sums         the weight of a cell split ONCE into sign, exponent and integer; per threshold the cells of a chunk that share
//                      an object and a bin are summed inside the wavefront and leave as ONE integer atomic; the field likewise;
//   k_obj_sums_finish  a thread per sum: the bins into one integer, ONE rounding to float64 (obj_sum_round).
// With the match (cpol_objects_match; MATCH of the header) behind all of them, on the piece arrays of the scratch (a second ObjArgs
// whose L, aux, rowcnt, table and n_objects are the pieces', n_maps = n_blocks * n_thr, min_area 1, max_objects = max_pieces, on a
// grid without the observed map's source):
//   k_match_runs   a wavefront per (block, row): the overlap flag of a cell from the two (root, number) lookups in the objects' L
//                  and aux (never the `labels` output); the piece L = the first cell of the cell's run in I, from the ballot as in
//                  k_obj_runs; `covered` with ONE integer atomic per run segment and side;
//   k_obj_merge, k_obj_flatten, k_obj_area, k_obj_count, k_obj_number   unchanged: they read of ObjArgs only f.row_groups, f.n_x,
//                  f.n_y, f.n_thr, f.cells, L, aux, rowcnt, table, n_objects, n_maps, connectivity, min_area and max_objects;
//   k_match_attr   per run segment the sums and the box as in k_obj_attr; the piece's root lane stores `forecast` and `observed`;
//   k_match_decode a thread per piece row: x0 out of its complement, y0 from the first cell.
// With the track (cpol_objects_track; TRACK of the header) behind all of them, on piece arrays of its own: k_track_bits,
// k_track_corr, k_track_shift, k_track_runs, the five kernels above unchanged, k_track_attr, k_match_decode (at the end of this file).

struct ObjArgs {
    FracArgs f;                     // the maps: plane, obs, domain, the grid, the rounded thresholds
    unsigned *L, *aux, *rowcnt;     // scratch (cpol_obj.h, ObjPlan)
    unsigned *n_objects;            // [n_maps]
    unsigned *table;                // [n_maps][max_objects][OBJ_WORDS]: zero before k_obj_number
    int *labels;                    // [n_maps][cells] or NULL
    long n_maps;
    int connectivity, min_area, max_objects;
    // the exact sums (NULL acc: off)
    unsigned long long *acc;        // [n_maps * max_objects + n_blocks + 1][OBJ_SUM_BINS]: zero before k_obj_sums
    double *volume;                 // [n_maps][max_objects][3]
    unsigned *skipped;              // [n_maps][max_objects]: zero before k_obj_sums
    double *field;                  // [n_blocks + 1][3]
    unsigned *field_cells;          // [n_blocks + 1][2]: zero before k_obj_sums
    const float *wv;                // the weight table on the device: breakpoints ...
    const double *wf;               // ... and values [n_weight]; n_weight 0: w = m
    int n_weight, step_w;           // step_w: the largest power of two <= n_weight
};

// the wavefront's source and row; false: no row (whole wavefronts leave: no barrier in these kernels)
__device__ __forceinline__ bool obj_row(const ObjArgs &a, long *src, int *y)
{
    *src = (long)blockIdx.x / a.f.row_groups;
    *y = (int)((long)blockIdx.x % a.f.row_groups) * OBJ_ROWS + (int)(threadIdx.x >> 6);
    return *y < a.f.n_y;
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_runs(const ObjArgs a)
{
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;
    const int n_x = a.f.n_x;
    const float *const row_in = (src < a.f.n_blocks ? a.f.plane + src * a.f.plane_stride : a.f.obs) + (long)y * n_x;
    const unsigned char *const row_dom = a.f.domain ? a.f.domain + (long)y * n_x : nullptr;
    unsigned *const row_out = a.L + src * a.f.n_thr * a.f.cells + (long)y * n_x;
    int carry[FRAC_MAX_THR] = {-1, -1, -1, -1};
    for (int x0 = 0; x0 < n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < n_x;
        const float v = in ? row_in[x] : 0.f;
        const bool d = in && (!row_dom || row_dom[x] != 0);
#pragma unroll
        for (int t = 0; t < FRAC_MAX_THR; ++t) {
            if (t >= a.f.n_thr) break;
            const bool set = d && v == v && v >= a.f.thr[t];
            const unsigned long long m = __ballot(set);
            unsigned first = OBJ_NONE;
            if (set) first = (unsigned)(y * n_x + (obj_run_open(m, lane) && carry[t] >= 0 ? carry[t] : x0 + obj_run_first(m, lane)));
            if (in) row_out[t * (long)a.f.cells + x] = first;
            carry[t] = obj_carry(m, x0, carry[t]);
        }
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_merge(const ObjArgs a)
{
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y) || y == 0) return;
    for (int t = 0; t < a.f.n_thr; ++t) {
        unsigned *const L = a.L + (src * a.f.n_thr + t) * a.f.cells;
        for (int x = lane; x < a.f.n_x; x += 64) obj_merge_cell(L, a.f.n_x, y, x, a.connectivity);
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_flatten(const ObjArgs a)
{
    const long i = (long)blockIdx.x * OBJ_THREADS + threadIdx.x;
    if (i >= a.n_maps * a.f.cells) return;
    a.aux[i] = 0u;
    if (a.L[i] == OBJ_NONE) return;
    const long map = i / a.f.cells;
    const unsigned *const L = a.L + map * a.f.cells;
    // (other threads flatten their cells meanwhile: a chain only gets shorter, and no root changes in this launch)
    a.L[i] = obj_find(L, (unsigned)(i - map * a.f.cells));
}

// what the later kernels read of a chunk: the cell's root and the ballot of the set cells
#define OBJ_CHUNK(t)                                                                                        \
    const long base = (src * a.f.n_thr + (t)) * a.f.cells;                                                 \
    const unsigned root = in ? a.L[base + cell] : OBJ_NONE;                                                 \
    const bool set = root != OBJ_NONE;                                                                      \
    const unsigned long long m = __ballot(set)

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_area(const ObjArgs a)
{
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;
    for (int x0 = 0; x0 < a.f.n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < a.f.n_x;
        const unsigned cell = (unsigned)(y * a.f.n_x + x);
        for (int t = 0; t < a.f.n_thr; ++t) {
            OBJ_CHUNK(t);
            // (the cells of a run share their root: the lane at which a run begins in the chunk adds the run's cells of the chunk)
            if (set && (lane == 0 || !((m >> (lane - 1)) & 1ull))) atomicAdd(a.aux + base + root, (unsigned)obj_run_len(m, lane));
        }
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_count(const ObjArgs a)
{
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;
    unsigned n[FRAC_MAX_THR] = {0u, 0u, 0u, 0u};
    for (int x0 = 0; x0 < a.f.n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < a.f.n_x;
        const unsigned cell = (unsigned)(y * a.f.n_x + x);
#pragma unroll
        for (int t = 0; t < FRAC_MAX_THR; ++t) {
            if (t >= a.f.n_thr) break;
            OBJ_CHUNK(t);
            (void)m;
            const bool keep = set && root == cell && a.aux[base + cell] >= (unsigned)a.min_area;
            n[t] += (unsigned)__popcll(__ballot(keep));
        }
    }
#pragma unroll
    for (int t = 0; t < FRAC_MAX_THR; ++t) {
        if (t >= a.f.n_thr) break;
        if (lane == 0) a.rowcnt[(src * a.f.n_thr + t) * a.f.n_y + y] = n[t];
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_number(const ObjArgs a)
{
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;
    const unsigned long long below = ~0ull >> (63 - lane);    // the lanes at or below this one
    unsigned carry[FRAC_MAX_THR];
#pragma unroll
    for (int t = 0; t < FRAC_MAX_THR; ++t) {
        carry[t] = 0u;
        if (t >= a.f.n_thr) continue;
        // the kept roots of the rows above: at most 1023 counts, summed by the wavefront
        const unsigned *const rc = a.rowcnt + (src * a.f.n_thr + t) * a.f.n_y;
        unsigned s = 0u;
        for (int r = lane; r < y; r += 64) s += rc[r];
        for (int dlt = 32; dlt > 0; dlt >>= 1) s += __shfl_xor(s, dlt);
        carry[t] = s;
    }
    for (int x0 = 0; x0 < a.f.n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < a.f.n_x;
        const unsigned cell = (unsigned)(y * a.f.n_x + x);
#pragma unroll
        for (int t = 0; t < FRAC_MAX_THR; ++t) {
            if (t >= a.f.n_thr) break;
            OBJ_CHUNK(t);
            (void)m;
            const bool is_root = set && root == cell;
            const unsigned area = is_root ? a.aux[base + cell] : 0u;
            const bool keep = is_root && area >= (unsigned)a.min_area;
            const unsigned long long k = __ballot(keep);
            const unsigned number = carry[t] + (unsigned)__popcll(k & below);       // 1-based: the lane itself counts
            if (is_root) a.aux[base + cell] = keep ? number : 0u;                 // (read by k_obj_attr, the next launch)
            if (keep && number <= (unsigned)a.max_objects) {
                unsigned *const row = a.table + ((src * a.f.n_thr + t) * a.max_objects + (number - 1u)) * OBJ_WORDS;
                row[OBJ_FIRST] = cell;
                row[OBJ_AREA] = area;
            }
            carry[t] += (unsigned)__popcll(k);
        }
    }
#pragma unroll
    for (int t = 0; t < FRAC_MAX_THR; ++t) {
        if (t >= a.f.n_thr) break;
        if (y == a.f.n_y - 1 && lane == 0) a.n_objects[src * a.f.n_thr + t] = carry[t];
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_attr(const ObjArgs a)
{
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;
    const int n_x = a.f.n_x;
    const float *const row_in = (src < a.f.n_blocks ? a.f.plane + src * a.f.plane_stride : a.f.obs) + (long)y * n_x;
    for (int x0 = 0; x0 < n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < n_x;
        const unsigned cell = (unsigned)(y * n_x + x);
        const unsigned bits = in ? __float_as_uint(row_in[x]) : 0u;
        for (int t = 0; t < a.f.n_thr; ++t) {
            OBJ_CHUNK(t);
            const unsigned number = set ? a.aux[base + root] : 0u;
            if (a.labels && in) a.labels[base + cell] = (int)number;
            // the peak of the run's cells of the chunk at the lane where they begin: after the step `dlt` a lane holds the maximum of
            // the 2 * dlt cells from itself on, cut at the end of its run
            const int len = set ? obj_run_len(m, lane) : 0;
            unsigned long long key = set ? obj_peak_key(bits, cell) : 0ull;
            for (int dlt = 1; dlt < 64; dlt <<= 1) {
                const unsigned long long other = __shfl_down(key, dlt);
                if (dlt < len && other > key) key = other;
            }
            if (!set || (lane != 0 && ((m >> (lane - 1)) & 1ull)) || number == 0u || number > (unsigned)a.max_objects) continue;
            unsigned *const row = a.table + ((src * a.f.n_thr + t) * a.max_objects + (number - 1u)) * OBJ_WORDS;
            const unsigned n = (unsigned)len, ux = (unsigned)x, uy = (unsigned)y;
            atomicAdd(row + OBJ_SUM_X, n * ux + n * (n - 1u) / 2u);
            atomicAdd(row + OBJ_SUM_Y, n * uy);
            atomicMax(row + OBJ_X0, (unsigned)(n_x - 1) - ux);                      // (a minimum as the maximum of the complement: the
            atomicMax(row + OBJ_X1, ux + n - 1u);                                  // table starts at zero; k_obj_decode turns it back)
            atomicMax(row + OBJ_Y1, uy);
            atomicMax((unsigned long long *)(row + OBJ_PEAK_CELL), key);
        }
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_decode(const ObjArgs a)
{
    const long i = (long)blockIdx.x * OBJ_THREADS + threadIdx.x;
    if (i >= a.n_maps * a.max_objects) return;
    const long map = i / a.max_objects;
    if ((unsigned)(i - map * a.max_objects) >= a.n_objects[map]) return;
    unsigned *const row = a.table + i * OBJ_WORDS;
    row[OBJ_X0] = (unsigned)(a.f.n_x - 1) - row[OBJ_X0];
    row[OBJ_Y0] = row[OBJ_FIRST] / (unsigned)a.f.n_x;         // (the first cell is the smallest flat index: it lies in the top row)
    const unsigned lo = row[OBJ_PEAK_CELL], hi = row[OBJ_PEAK_BITS];
    row[OBJ_PEAK_CELL] = ~lo;
    row[OBJ_PEAK_BITS] = obj_unorder(hi);
}

// ---- the exact sums ----

__device__ __forceinline__ long long obj_wave_sum(long long v)
{
    for (int dlt = 32; dlt > 0; dlt >>= 1) v += __shfl_xor(v, dlt);
    return v;
}

// The lanes with `on` hold a key (accumulator row << 5 | bin of the moments, E >> 3; the volume's bin is half of it) and three
// signed contributions.  While lanes remain: the first remaining lane's key, the ballot of the lanes with the same key, their
// contributions summed across the wavefront (at most 64 terms below 2^41: no overflow), ONE atomic per sum by that lane.
// TERMINATION: `left` is the same in every lane (a ballot) and loses at least the leading lane's bit in every turn: at most 64
// turns.  Every lane of the wavefront calls this together.
__device__ __forceinline__ void obj_sums_combine(unsigned long long *rows, bool on, unsigned key, long long cv, long long cx, long long cy, int lane)
{
    unsigned long long left = __ballot(on);
    while (left) {
        const int lead = __builtin_ctzll(left);
        const unsigned k = __shfl(key, lead);
        const bool mine = on && key == k;
        const long long sv = obj_wave_sum(mine ? cv : 0ll), sx = obj_wave_sum(mine ? cx : 0ll), sy = obj_wave_sum(mine ? cy : 0ll);
        if (lane == lead) {
            unsigned long long *const row = rows + (size_t)(k >> 5) * OBJ_SUM_BINS;
            const unsigned b = k & 31u;
            if (sv) atomicAdd(row + (b >> 1), (unsigned long long)sv);
            if (sx) atomicAdd(row + OBJ_SUM_VOL_BINS + b, (unsigned long long)sx);
            if (sy) atomicAdd(row + OBJ_SUM_VOL_BINS + OBJ_SUM_MOM_BINS + b, (unsigned long long)sy);
        }
        left &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_sums(const ObjArgs a)
{
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;
    const int n_x = a.f.n_x;
    const float *const row_in = (src < a.f.n_blocks ? a.f.plane + src * a.f.plane_stride : a.f.obs) + (long)y * n_x;
    const unsigned char *const row_dom = a.f.domain ? a.f.domain + (long)y * n_x : nullptr;
    unsigned long long *const field_row = a.acc + ((size_t)a.n_maps * a.max_objects + src) * OBJ_SUM_BINS;
    unsigned n_summed = 0u, n_skipped = 0u;
    for (int x0 = 0; x0 < n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < n_x;
        const unsigned cell = (unsigned)(y * n_x + x);
        const float v = in ? row_in[x] : 0.f;
        const bool d = in && (!row_dom || row_dom[x] != 0) && v == v;
        const float w = d && a.n_weight ? obj_weight(a.wv, a.wf, a.n_weight, a.step_w, v) : v;
        const unsigned bits = __float_as_uint(w);
        int E; unsigned M;
        const bool finite = obj_sum_split(bits, &E, &M);
        const bool sum = d && finite, skip = d && !finite;
        const long long cv = sum ? obj_sum_term(bits, M, 1u, E & 15) : 0ll;
        const long long cx = sum ? obj_sum_term(bits, M, (unsigned)x, E & 7) : 0ll;
        const long long cy = sum ? obj_sum_term(bits, M, (unsigned)y, E & 7) : 0ll;
        const unsigned bin = (unsigned)(E >> 3);
        n_summed += (unsigned)__popcll(__ballot(sum));
        n_skipped += (unsigned)__popcll(__ballot(skip));
        obj_sums_combine(field_row, sum, bin, cv, cx, cy, lane);                    // (row 0 of field_row: the source's own)
        for (int t = 0; t < a.f.n_thr; ++t) {
            OBJ_CHUNK(t);
            (void)m;
            const unsigned number = set ? a.aux[base + root] : 0u;
            const bool kept = number != 0u && number <= (unsigned)a.max_objects;    // (a set cell lies in the domain and is no NaN)
            const long map = src * a.f.n_thr + t;
            obj_sums_combine(a.acc + (size_t)map * a.max_objects * OBJ_SUM_BINS, kept && sum, ((number - 1u) << 5) | bin, cv, cx, cy, lane);
            if (kept && skip) atomicAdd(a.skipped + map * a.max_objects + (number - 1u), 1u);
        }
    }
    if (lane == 0) {
        if (n_summed) atomicAdd(a.field_cells + 2 * src, n_summed);
        if (n_skipped) atomicAdd(a.field_cells + 2 * src + 1, n_skipped);
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_sums_finish(const ObjArgs a)
{
    const long i = (long)blockIdx.x * OBJ_THREADS + threadIdx.x;
    const long n_rows = a.n_maps * a.max_objects;
    if (i >= (n_rows + a.f.n_blocks + 1) * 3) return;
    const long r = i / 3;
    const int which = (int)(i - r * 3);
    const unsigned long long *const row = a.acc + (size_t)r * OBJ_SUM_BINS;
    // (the rows at or beyond n_objects took no atomic: +0.0)
    const unsigned long long bits = which == 0 ? obj_sum_round(row, OBJ_SUM_VOL_BINS, 16)
                                               : obj_sum_round(row + OBJ_SUM_VOL_BINS + (which - 1) * OBJ_SUM_MOM_BINS, OBJ_SUM_MOM_BINS, 8);
    double *const out = r < n_rows ? a.volume + r * 3 : a.field + (r - n_rows) * 3;
    out[which] = __longlong_as_double((long long)bits);
}

// ---- the match ----

struct MatchArgs {
    ObjArgs p;                      // the pieces: f as the objects', L, aux, rowcnt the piece scratch, table = pieces, n_objects = n_pieces
    const unsigned *L, *aux;        // the objects' arrays after k_obj_number: L flattened, aux[root] = the kept number or 0
    unsigned *covered;              // [n_blocks * n_thr][2][max_objects]: zero before k_match_runs
    int max_objects;
};

__global__ __launch_bounds__(OBJ_THREADS) void k_match_runs(const MatchArgs g)
{
    const ObjArgs &a = g.p;
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;                    // (the grid has n_blocks sources: src is a block)
    const int n_x = a.f.n_x;
    int carry[FRAC_MAX_THR] = {-1, -1, -1, -1};
    for (int x0 = 0; x0 < n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < n_x;
        const unsigned cell = (unsigned)(y * n_x + x);
#pragma unroll
        for (int t = 0; t < FRAC_MAX_THR; ++t) {
            if (t >= a.f.n_thr) break;
            const long map = src * a.f.n_thr + t;
            const long fb = map * a.f.cells, ob = ((long)a.f.n_blocks * a.f.n_thr + t) * a.f.cells;
            unsigned nf = 0u, no = 0u;
            const bool set = in && obj_match_flag(g.L + fb, g.aux + fb, g.L + ob, g.aux + ob, cell, &nf, &no);
            const unsigned long long m = __ballot(set);
            unsigned first = OBJ_NONE;
            if (set) first = (unsigned)(y * n_x + (obj_run_open(m, lane) && carry[t] >= 0 ? carry[t] : x0 + obj_run_first(m, lane)));
            if (in) a.L[fb + cell] = first;
            if (set && (lane == 0 || !((m >> (lane - 1)) & 1ull)))
                obj_match_cover(g.covered + map * 2 * g.max_objects, g.max_objects, nf, no, (unsigned)obj_run_len(m, lane));
            carry[t] = obj_carry(m, x0, carry[t]);
        }
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_match_attr(const MatchArgs g)
{
    const ObjArgs &a = g.p;
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;
    const int n_x = a.f.n_x;
    for (int x0 = 0; x0 < n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < n_x;
        const unsigned cell = (unsigned)(y * n_x + x);
        for (int t = 0; t < a.f.n_thr; ++t) {
            OBJ_CHUNK(t);
            const unsigned number = set ? a.aux[base + root] : 0u;
            if (!set || number == 0u || number > (unsigned)a.max_objects) continue;
            unsigned *const row = a.table + ((src * a.f.n_thr + t) * a.max_objects + (number - 1u)) * OBJ_WORDS;
            if (root == cell) {                               // (one lane per piece: plain stores)
                const long ob = ((long)a.f.n_blocks * a.f.n_thr + t) * a.f.cells;
                row[OBJ_PEAK_CELL] = obj_number_of(g.L + base, g.aux + base, cell);
                row[OBJ_PEAK_BITS] = obj_number_of(g.L + ob, g.aux + ob, cell);
            }
            if (lane != 0 && ((m >> (lane - 1)) & 1ull)) continue;
            const unsigned n = (unsigned)obj_run_len(m, lane), ux = (unsigned)x, uy = (unsigned)y;
            atomicAdd(row + OBJ_SUM_X, n * ux + n * (n - 1u) / 2u);
            atomicAdd(row + OBJ_SUM_Y, n * uy);
            atomicMax(row + OBJ_X0, (unsigned)(n_x - 1) - ux);                      // (k_match_decode turns it back)
            atomicMax(row + OBJ_X1, ux + n - 1u);
            atomicMax(row + OBJ_Y1, uy);
        }
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_match_decode(const MatchArgs g)
{
    const ObjArgs &a = g.p;
    const long i = (long)blockIdx.x * OBJ_THREADS + threadIdx.x;
    if (i >= a.n_maps * a.max_objects) return;
    const long map = i / a.max_objects;
    if ((unsigned)(i - map * a.max_objects) >= a.n_objects[map]) return;
    unsigned *const row = a.table + i * OBJ_WORDS;
    row[OBJ_X0] = (unsigned)(a.f.n_x - 1) - row[OBJ_X0];
    row[OBJ_Y0] = row[OBJ_FIRST] / (unsigned)a.f.n_x;
}

// ---- the track (cpol_objects_track; TRACK of the header): block p against block p + 1, the earlier one shifted.  Behind
// everything else; the piece arrays are the track's own (a third ObjArgs: n_maps = (n_blocks - 1) * n_thr, on a grid of
// n_blocks - 1 sources), so the match against the observed map beside it changes nothing.
//   k_track_bits   a wavefront per (block, row): Ke of every threshold from the (root, number) lookup, packed with the ballot;
//   k_track_corr   a workgroup per (pair, threshold, slab of OBJ_TRACK_ROWS earlier rows), a thread per counter (dy, dx) in turn:
//                  popcounts of earlier words against funnel-shifted later words in a register, ONE integer atomic per counter;
//   k_track_shift  a wavefront per (pair, threshold): the argmax as one 64-bit maximum (obj_track_key);
//   k_track_runs   k_match_runs with the earlier lookup at cell - shift, the shift read from device memory;
//   k_track_attr   k_match_attr likewise; then k_match_decode as it is.
struct TrackArgs {
    ObjArgs p;                      // the track's pieces, as MatchArgs::p
    const unsigned *L, *aux;        // the objects' arrays after k_obj_number
    unsigned *covered;              // [n_pairs * n_thr][2][max_objects]: zero before k_track_runs
    int max_objects;
    unsigned long long *bits;       // [n_blocks * n_thr][n_y][words]
    unsigned *corr;                 // [n_pairs * n_thr][side][side]: zero before k_track_corr (NULL: the shifts are given)
    int *shift;                     // [n_pairs * n_thr][2]
    int S, side, words, slabs;
    long track_maps;
};

__global__ __launch_bounds__(OBJ_THREADS) void k_track_bits(const TrackArgs g)
{
    const ObjArgs &a = g.p;
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;                    // (the grid has n_blocks sources)
    const int n_x = a.f.n_x;
    for (int x0 = 0; x0 < n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < n_x;
        const unsigned cell = (unsigned)(y * n_x + x);
        for (int t = 0; t < a.f.n_thr; ++t) {
            const long map = src * a.f.n_thr + t, fb = map * a.f.cells;
            const unsigned long long m = __ballot(in && obj_number_of(g.L + fb, g.aux + fb, cell) != 0u);
            if (lane == 0) g.bits[(map * a.f.n_y + y) * g.words + (x0 >> 6)] = m;
        }
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_track_corr(const TrackArgs g)
{
    const ObjArgs &a = g.p;
    const long map = (long)blockIdx.x / g.slabs;          // pair p, threshold t: map p * n_thr + t
    const int y0 = (int)((long)blockIdx.x % g.slabs) * OBJ_TRACK_ROWS;
    const int y1 = y0 + OBJ_TRACK_ROWS < a.f.n_y ? y0 + OBJ_TRACK_ROWS : a.f.n_y;
    const long per = (long)a.f.n_y * g.words;
    const unsigned long long *const ke = g.bits + map * per, *const kl = ke + a.f.n_thr * per;   // (block p + 1, the same threshold)
    unsigned *const out = g.corr + map * g.side * g.side;
    for (int c = (int)threadIdx.x; c < g.side * g.side; c += OBJ_THREADS) {
        const unsigned n = obj_track_count(ke, kl, a.f.n_y, g.words, y0, y1, c / g.side - g.S, c % g.side - g.S);
        if (n) atomicAdd(out + c, n);
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_track_shift(const TrackArgs g)
{
    const int lane = threadIdx.x & 63;
    const long map = (long)blockIdx.x * OBJ_ROWS + (long)(threadIdx.x >> 6);
    if (map >= g.track_maps) return;                      // (whole wavefronts leave)
    const unsigned *const in = g.corr + map * g.side * g.side;
    unsigned long long best = 0ull;                       // (below every key: a key's low word is never 0)
    for (int c = lane; c < g.side * g.side; c += 64) {
        const unsigned long long key = obj_track_key(in[c], c / g.side - g.S, c % g.side - g.S, g.S);
        if (key > best) best = key;
    }
    for (int dlt = 32; dlt > 0; dlt >>= 1) {
        const unsigned long long other = __shfl_xor(best, dlt);
        if (other > best) best = other;
    }
    if (lane == 0) {
        int dy, dx;
        obj_track_unkey(best, g.S, &dy, &dx);
        g.shift[2 * map] = dy;
        g.shift[2 * map + 1] = dx;
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_track_runs(const TrackArgs g)
{
    const ObjArgs &a = g.p;
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;                    // (the grid has n_blocks - 1 sources: src is a pair)
    const int n_x = a.f.n_x;
    int carry[FRAC_MAX_THR] = {-1, -1, -1, -1};
    for (int x0 = 0; x0 < n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < n_x;
        const unsigned cell = (unsigned)(y * n_x + x);
#pragma unroll
        for (int t = 0; t < FRAC_MAX_THR; ++t) {
            if (t >= a.f.n_thr) break;
            const long map = src * a.f.n_thr + t;
            const long eb = map * a.f.cells, lb = eb + (long)a.f.n_thr * a.f.cells;      // the earlier block's map, the later one's
            const int dy = g.shift[2 * map], dx = g.shift[2 * map + 1];
            const unsigned ne = in ? obj_track_number(g.L + eb, g.aux + eb, n_x, a.f.n_y, y, x, dy, dx) : 0u;
            const unsigned nl = in ? obj_number_of(g.L + lb, g.aux + lb, cell) : 0u;
            const bool set = ne != 0u && nl != 0u;
            const unsigned long long m = __ballot(set);
            unsigned first = OBJ_NONE;
            if (set) first = (unsigned)(y * n_x + (obj_run_open(m, lane) && carry[t] >= 0 ? carry[t] : x0 + obj_run_first(m, lane)));
            if (in) a.L[eb + cell] = first;
            // (a run of the overlap lies inside one run of each map, shifted or not: ne and nl are constant over it)
            if (set && (lane == 0 || !((m >> (lane - 1)) & 1ull)))
                obj_match_cover(g.covered + map * 2 * g.max_objects, g.max_objects, ne, nl, (unsigned)obj_run_len(m, lane));
            carry[t] = obj_carry(m, x0, carry[t]);
        }
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_track_attr(const TrackArgs g)
{
    const ObjArgs &a = g.p;
    const int lane = threadIdx.x & 63;
    long src; int y;
    if (!obj_row(a, &src, &y)) return;
    const int n_x = a.f.n_x;
    for (int x0 = 0; x0 < n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < n_x;
        const unsigned cell = (unsigned)(y * n_x + x);
        for (int t = 0; t < a.f.n_thr; ++t) {
            OBJ_CHUNK(t);
            const unsigned number = set ? a.aux[base + root] : 0u;
            if (!set || number == 0u || number > (unsigned)a.max_objects) continue;
            const long map = src * a.f.n_thr + t;
            unsigned *const row = a.table + (map * a.max_objects + (number - 1u)) * OBJ_WORDS;
            if (root == cell) {                               // (one lane per piece: plain stores)
                const long lb = base + (long)a.f.n_thr * a.f.cells;
                row[OBJ_PEAK_CELL] = obj_track_number(g.L + base, g.aux + base, n_x, a.f.n_y, y, x, g.shift[2 * map], g.shift[2 * map + 1]);
                row[OBJ_PEAK_BITS] = obj_number_of(g.L + lb, g.aux + lb, cell);
            }
            if (lane != 0 && ((m >> (lane - 1)) & 1ull)) continue;
            const unsigned n = (unsigned)obj_run_len(m, lane), ux = (unsigned)x, uy = (unsigned)y;
            atomicAdd(row + OBJ_SUM_X, n * ux + n * (n - 1u) / 2u);
            atomicAdd(row + OBJ_SUM_Y, n * uy);
            atomicMax(row + OBJ_X0, (unsigned)(n_x - 1) - ux);                      // (k_match_decode turns it back)
            atomicMax(row + OBJ_X1, ux + n - 1u);
            atomicMax(row + OBJ_Y1, uy);
        }
    }
}

#undef OBJ_CHUNK
