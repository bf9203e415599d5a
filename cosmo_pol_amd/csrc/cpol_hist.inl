// cpol_hist.inl -- sweep histograms: counts of the per-gate fields of a call over many gates (cpol_histogram).
//
// Reference functions replaced (wolfidan/cosmo_pol): none -- the reference hands back per-gate radials, and its users call
// np.histogram2d on them.  The rule is the one of include/cosmo_pol_amd.h and cosmo_pol_amd/histogram.py (`count`): the bin
// of a value is the number of edges at or below it, found by comparisons alone, and the result is a sum of integers -- whatever
// order the hardware adds in, the counts are those of NumPy.  No float atomics, no arithmetic on the values.

struct HistArgs {
    const void *x;                  // the field [n_rows * n_gates], TX
    const void *y;                  // the ordinate [y_gates], TY (NULL without one)
    const void *ex, *ey;            // the rounded edges on the device, TX [n_ex] and TY [n_ey]
    unsigned long long *state;      // this field's table of the running state: [n_blocks][cells]
    long block_gates;               // rows_per_block * n_gates: the gates of one block
    long y_gates;                   // the gates the ordinate array holds (the geometry of an ensemble call: once); gate g reads g % y_gates
    int n_ex, n_ey;                 // edges (n + 1)
    int step_x, step_y;             // the largest power of two <= n_ex / n_ey: the first step of the search
    int nx2;                        // n_x + 2: the cells of one ordinate row
    int cells;                      // (n_x + 2) * (n_y + 2)
    int stretches;                  // stretches of one block
};

// #{ j : e[j] <= v } for n ascending edges in LDS, branch-free: one comparison per step, steps step0, step0 / 2, ... 1 with step0
// the largest power of two <= n -- floor(log2 n) + 1 comparisons, 10 up to 1023 edges (11 at the limit of 1024, whose 1025
// outcomes no 10 comparisons can tell apart).  A NaN compares false everywhere and gives 0; such a gate does not count anyway.
template <typename T>
__device__ __forceinline__ int hist_bin(const T *e, int n, int step0, T v)
{
    int lo = 0;
    for (int step = step0; step > 0; step >>= 1) {
        const int t = lo + step;
        const T edge = e[min(t, n) - 1];
        lo = (t <= n && edge <= v) ? t : lo;
    }
    return lo;
}

template <typename T> struct HistNone { static constexpr bool none = false; typedef T type; };
template <> struct HistNone<void> { static constexpr bool none = true; typedef float type; };

// A workgroup owns one stretch of HIST_STRETCH gates of ONE block and ONE field (a launch per requested field) and never
// crosses a block boundary: its table lives in LDS as uint32 (a stretch is far below 2^32 gates), the rounded edges of both axes
// beside it.  Zero, barrier, count with LDS integer atomics, barrier, then only the non-zero cells go to the context's uint64
// state, one no-return 64-bit global integer atomic each.
template <typename TX, typename TYV>
__global__ __launch_bounds__(HIST_THREADS) void k_hist(const HistArgs a)
{
    typedef typename HistNone<TYV>::type TY;
    constexpr bool with_y = !HistNone<TYV>::none;
    extern __shared__ unsigned long long hist_lds[];            // (8-byte aligned: the float64 edges come first)
    const int tid = threadIdx.x;
    const int px = (a.n_ex * (int)sizeof(TX) + 7) / 8, py = with_y ? (a.n_ey * (int)sizeof(TY) + 7) / 8 : 0;
    TX *const ex = (TX *)hist_lds;
    TY *const ey = (TY *)(hist_lds + px);
    unsigned *const tab = (unsigned *)(hist_lds + px + py);
    for (int j = tid; j < a.n_ex; j += HIST_THREADS) ex[j] = ((const TX *)a.ex)[j];
    if (with_y)
        for (int j = tid; j < a.n_ey; j += HIST_THREADS) ey[j] = ((const TY *)a.ey)[j];
    for (int c = tid; c < a.cells; c += HIST_THREADS) tab[c] = 0u;
    __syncthreads();
    const long b = (long)blockIdx.x / a.stretches;
    const long s = (long)blockIdx.x % a.stretches;
    const long g0 = b * a.block_gates + s * (long)HIST_STRETCH;
    const long g1 = min(g0 + (long)HIST_STRETCH, (b + 1) * a.block_gates);
    const TX *const x = (const TX *)a.x;
    const TY *const y = (const TY *)a.y;
    for (long g = g0 + tid; g < g1; g += HIST_THREADS) {
        const TX v = x[g];
        bool counts = v == v;
        int cell = hist_bin<TX>(ex, a.n_ex, a.step_x, v);
        if (with_y) {
            const TY w = y[g < a.y_gates ? g : g % a.y_gates];      // (the geometry of an ensemble call: n_rays rows once)
            counts = counts && w == w;
            cell += hist_bin<TY>(ey, a.n_ey, a.step_y, w) * a.nx2;
        }
        if (counts) atomicAdd(&tab[cell], 1u);
    }
    __syncthreads();
    unsigned long long *const out = a.state + b * (long)a.cells;
    for (int c = tid; c < a.cells; c += HIST_THREADS) {
        const unsigned n = tab[c];
        if (n) atomicAdd(&out[c], (unsigned long long)n);
    }
}

// the launch of one field's instantiation (grid 0: none) and its address (for hipFuncSetAttribute)
template <typename TX>
static void hist_launch_typed(int ord_type, unsigned grid, size_t lds, hipStream_t st, const HistArgs &ha, const void **fn)
{
    if (ord_type == HIST_T_NONE) { *fn = (const void *)k_hist<TX, void>; if (grid) hipLaunchKernelGGL((k_hist<TX, void>), dim3(grid), dim3(HIST_THREADS), lds, st, ha); }
    else if (ord_type == HIST_T_F32) { *fn = (const void *)k_hist<TX, float>; if (grid) hipLaunchKernelGGL((k_hist<TX, float>), dim3(grid), dim3(HIST_THREADS), lds, st, ha); }
    else { *fn = (const void *)k_hist<TX, double>; if (grid) hipLaunchKernelGGL((k_hist<TX, double>), dim3(grid), dim3(HIST_THREADS), lds, st, ha); }
}

static void hist_launch_field(bool x64, int ord_type, unsigned grid, size_t lds, hipStream_t st, const HistArgs &ha, const void **fn)
{
    if (x64) hist_launch_typed<double>(ord_type, grid, lds, st, ha, fn);
    else hist_launch_typed<float>(ord_type, grid, lds, st, ha, fn);
}
