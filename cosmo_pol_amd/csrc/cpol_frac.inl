// cpol_frac.inl -- neighbourhood verification: the sums of the fractions skill score of one finished plane of a composite
// against an observed map, per block, threshold and neighbourhood size (cpol_fractions).
//
// Reference functions replaced (wolfidan/cosmo_pol): none -- the reference hands back per-gate radials; a verification group
// grids them, thresholds forecast and observation and runs box filters on the host.  The rule is the one of
// include/cosmo_pol_amd.h and cosmo_pol_amd/neighbourhood.py (`sums`): float32 comparisons make the binary maps, and from there
// on every number is an INTEGER -- counts of set cells in uint32 summed-area tables, squares and their sums in uint64 (the
// header derives that nothing overflows) -- so the sums are those of NumPy whatever order the hardware works in.  No float
// arithmetic, no compare-and-swap loops; the only atomics are 64-bit integer additions, one per workgroup and sum.
//
// Three launches behind k_comp_finish, on the plane where it lies:
//   k_frac_rows   a wavefront per (source, row): the binary maps of all thresholds from ONE read of the row, scanned along x;
//   k_frac_cols   a lane per (table, column) walking down y: the row scans become summed-area tables;
//   k_frac_score  a thread per cell and (block, threshold): four look-ups per table and radius, squares reduced across the
//                 workgroup, then added.
// The observation is source n_blocks: its tables are built once and read by every block.

struct FracArgs {
    const float *plane;             // block 0's plane [n_y][n_x]; block b's lies plane_stride floats further per block
    const float *obs;               // [n_y][n_x]
    const unsigned char *domain;    // [n_y][n_x] or NULL
    unsigned *sat;                  // [n_tables][n_y + 1][n_x + 1], table (s * n_thr + t) of source s and threshold t
    unsigned long long *sums;       // [n_blocks][n_thr][n_radii][3]: zero before k_frac_score
    unsigned long long *totals;     // [n_blocks][n_thr][3]: likewise
    long plane_stride;
    long table;                     // (n_y + 1) * (n_x + 1)
    long n_blocks;
    int n_x, n_y, cells;
    int n_thr, n_radii;
    int row_groups;                 // workgroups of k_frac_rows per source: ceil(n_y / FRAC_ROWS)
    int col_chunks;                 // workgroups of k_frac_cols per table: ceil(n_x / 64)
    int score_groups;               // workgroups of k_frac_score per (block, threshold): ceil(cells / FRAC_CELLS)
    float thr[FRAC_MAX_THR];        // rounded
    int radii[FRAC_MAX_RADII];
};

// A wavefront owns one row of one source and reads it once, in chunks of 64 cells.  A cell is set or not, so the scan of a chunk
// needs no shuffle network: the ballot of the chunk's flags, masked to the lanes at or below this one and counted, IS the
// inclusive prefix sum, and the count of the whole ballot is the carry into the next chunk -- two scalar-width integer
// instructions per threshold instead of six shuffle steps.  Entry [y + 1][x + 1] of the table takes the prefix; column 0 and row 0
// are written zero here, so no launch clears the tables.
__global__ __launch_bounds__(FRAC_THREADS) void k_frac_rows(const FracArgs a)
{
    const int lane = threadIdx.x & 63;
    const long src = (long)blockIdx.x / a.row_groups;
    const int y = (int)((long)blockIdx.x % a.row_groups) * FRAC_ROWS + (int)(threadIdx.x >> 6);
    if (y >= a.n_y) return;                                   // (whole wavefronts: no barrier in this kernel)
    const float *const row_in = (src < a.n_blocks ? a.plane + src * a.plane_stride : a.obs) + (long)y * a.n_x;
    const unsigned char *const row_dom = a.domain ? a.domain + (long)y * a.n_x : nullptr;
    const int W = a.n_x + 1;
    unsigned *const tab0 = a.sat + src * a.n_thr * a.table;
    unsigned *const row_out = tab0 + (long)(y + 1) * W;
    const unsigned long long below = ~0ull >> (63 - lane);    // the lanes at or below this one
    unsigned carry[FRAC_MAX_THR] = {0u, 0u, 0u, 0u};
    for (int x0 = 0; x0 < a.n_x; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < a.n_x;
        const float v = in ? row_in[x] : 0.f;
        const bool d = in && (!row_dom || row_dom[x] != 0);
#pragma unroll
        for (int t = 0; t < FRAC_MAX_THR; ++t) {
            if (t >= a.n_thr) break;
            const bool set = d && v == v && v >= a.thr[t];
            const unsigned long long m = __ballot(set);
            if (in) row_out[t * a.table + x + 1] = carry[t] + (unsigned)__popcll(m & below);
            carry[t] += (unsigned)__popcll(m);
        }
    }
#pragma unroll
    for (int t = 0; t < FRAC_MAX_THR; ++t) {
        if (t >= a.n_thr) break;
        if (lane == 0) row_out[t * a.table] = 0u;
        if (y == 0)
            for (int x = lane; x < W; x += 64) tab0[t * a.table + x] = 0u;
    }
}

// A lane owns one column of one table and walks down y adding the rows above: consecutive lanes read and write consecutive
// addresses of a row.  The loads do not depend on the running sum, so the unrolled loop keeps several in flight.
__global__ __launch_bounds__(64) void k_frac_cols(const FracArgs a)
{
    const long tab = (long)blockIdx.x / a.col_chunks;
    const int x = (int)((long)blockIdx.x % a.col_chunks) * 64 + (int)threadIdx.x;
    if (x >= a.n_x) return;
    const int W = a.n_x + 1;
    unsigned *p = a.sat + tab * a.table + W + x + 1;
    unsigned run = 0u;
#pragma unroll 4
    for (int y = 0; y < a.n_y; ++y, p += W) {
        run += *p;
        *p = run;
    }
}

// the set cells of a table inside rows [y0, y1) and columns [x0, x1): differences of uint32, exact modulo 2^32 and < 2^20
__device__ __forceinline__ unsigned frac_window(const unsigned *s, int W, int y0, int y1, int x0, int x1)
{
    return s[y1 * W + x1] - s[y0 * W + x1] - s[y1 * W + x0] + s[y0 * W + x0];
}

// A workgroup owns FRAC_CELLS consecutive cells of one (block, threshold), four per thread, strided so that a wavefront reads
// consecutive cells.  Per cell of the domain and radius: the window clipped to the grid, four look-ups in the block's table and
// four in the observation's, the three squares into uint64 registers.  Then a shuffle reduction inside the wavefront, the four
// wavefronts through LDS, and ONE atomic integer addition per sum and workgroup.
__global__ __launch_bounds__(FRAC_THREADS) void k_frac_score(const FracArgs a)
{
    __shared__ unsigned long long part[FRAC_THREADS / 64][3 * FRAC_MAX_RADII + 1];
    const int tid = threadIdx.x;
    const long bt = (long)blockIdx.x / a.score_groups;        // b * n_thr + t
    const int grp = (int)((long)blockIdx.x % a.score_groups);
    const int t = (int)(bt % a.n_thr);
    const int W = a.n_x + 1;
    const unsigned *const sf = a.sat + bt * a.table;
    const unsigned *const so = a.sat + (a.n_blocks * a.n_thr + t) * a.table;
    unsigned long long acc[FRAC_MAX_RADII][3];
#pragma unroll
    for (int w = 0; w < FRAC_MAX_RADII; ++w) acc[w][0] = acc[w][1] = acc[w][2] = 0ull;
    unsigned long long n_dom = 0ull;
#pragma unroll
    for (int i = 0; i < FRAC_CELLS / FRAC_THREADS; ++i) {
        const int cell = grp * FRAC_CELLS + i * FRAC_THREADS + tid;
        if (cell >= a.cells || (a.domain && a.domain[cell] == 0)) continue;
        const int y = cell / a.n_x, x = cell - y * a.n_x;
        ++n_dom;
#pragma unroll
        for (int w = 0; w < FRAC_MAX_RADII; ++w) {
            if (w >= a.n_radii) break;
            const int r = a.radii[w];
            const int y0 = max(y - r, 0), y1 = min(y + r, a.n_y - 1) + 1, x0 = max(x - r, 0), x1 = min(x + r, a.n_x - 1) + 1;
            const unsigned nf = frac_window(sf, W, y0, y1, x0, x1), no = frac_window(so, W, y0, y1, x0, x1);
            const long long d = (long long)nf - (long long)no;
            acc[w][0] += (unsigned long long)(d * d);
            acc[w][1] += (unsigned long long)nf * nf;
            acc[w][2] += (unsigned long long)no * no;
        }
    }
    // (every lane of the workgroup arrives here: the shuffles and the barrier need whole wavefronts)
#pragma unroll
    for (int w = 0; w < FRAC_MAX_RADII; ++w) {
        if (w >= a.n_radii) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            unsigned long long v = acc[w][k];
            for (int dlt = 32; dlt > 0; dlt >>= 1) v += __shfl_down(v, dlt);
            if ((tid & 63) == 0) part[tid >> 6][3 * w + k] = v;
        }
    }
    for (int dlt = 32; dlt > 0; dlt >>= 1) n_dom += __shfl_down(n_dom, dlt);
    if ((tid & 63) == 0) part[tid >> 6][3 * FRAC_MAX_RADII] = n_dom;
    __syncthreads();
    if (tid < 3 * a.n_radii) {
        unsigned long long v = 0ull;
        for (int q = 0; q < FRAC_THREADS / 64; ++q) v += part[q][tid];
        atomicAdd(&a.sums[bt * a.n_radii * 3 + tid], v);
    } else if (tid == 3 * FRAC_MAX_RADII) {
        unsigned long long v = 0ull;
        for (int q = 0; q < FRAC_THREADS / 64; ++q) v += part[q][tid];
        atomicAdd(&a.totals[bt * 3 + 2], v);
        // the last entry of a finished table is the number of its set cells
        if (grp == 0) {
            a.totals[bt * 3 + 0] = sf[a.table - 1];
            a.totals[bt * 3 + 1] = so[a.table - 1];
        }
    }
}
