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

struct ObjArgs {
    FracArgs f;                     // the maps: plane, obs, domain, the grid, the rounded thresholds
    unsigned *L, *aux, *rowcnt;     // scratch (cpol_obj.h, ObjPlan)
    unsigned *n_objects;            // [n_maps]
    unsigned *table;                // [n_maps][max_objects][OBJ_WORDS]: zero before k_obj_number
    int *labels;                    // [n_maps][cells] or NULL
    long n_maps;
    int connectivity, min_area, max_objects;
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

#undef OBJ_CHUNK
