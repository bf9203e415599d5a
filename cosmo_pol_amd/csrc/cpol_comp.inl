// cpol_comp.inl -- gridded composites: the column maximum, the lowest gate and echo-top heights of the per-gate fields of a call
// on a radar-centred map or on a plane of the caller's per-gate coordinates, of one radar or of a network (cpol_composite).
//
// Reference functions replaced (wolfidan/cosmo_pol): none -- the reference hands back per-gate radials, and its users compute per
// gate where it lies and scatter with np.maximum.at.  The rule is the one of include/cosmo_pol_amd.h and
// cosmo_pol_amd/composite.py (`compose`, `finish`): the cell of a gate is found by ONE float64 multiplication per axis (the
// caller gives sine and cosine) and comparisons alone, and every result is a maximum, a minimum or a sum of INTEGERS (the ordered
// keys of the float32 values) -- whatever order the hardware works in, the maps are those of NumPy.  No float atomics, no
// compare-and-swap loops, no trigonometric function.  The exact sums (CPOL_COMP_SUM: k_comp_sum, k_comp_sum_finish at the end of
// this file) keep to that: a float32 is an integer multiple of 2^-149, the sums are sums of integers, rounded once.

struct CompArgs {
    const float *v;                 // the field [n_rows * n_gates]
    const float *dist, *hgt;        // [geo_gates]
    const double *ex, *ey;          // the edges on the device [n_ex], [n_ey]
    const double *ray_sin, *ray_cos;   // [n_rays]
    unsigned long long *smax, *slow, *scount;  // this field's states [n_blocks][cells] (NULL: product not requested)
    unsigned *stop;                 // [n_blocks][n_thr][cells]
    long block_gates;               // rows_per_block * n_gates: the gates of one block
    long geo_gates;                 // the gates the geometry arrays hold (an ensemble call: n_rays rows once); gate g reads g % geo_gates
    int n_gates;
    int n_ex, n_ey;                 // edges (n + 1)
    int step_x, step_y;             // the largest power of two <= n_ex / n_ey: the first step of the search
    int n_x, n_y, cells;            // cells = n_x * n_y
    int stretches;                  // stretches of one block
    int n_thr, slab;
    float h_lo, h_hi;
    float thr[COMP_MAX_THR];        // rounded
    const double *gx, *gy;          // the gate plane: the caller's x and y [geo_gates] (the radar plane reads neither)
    const float *ez;                // LAYERS: the rounded layer edges on the device [n_z + 1]
    long block_cells;               // LAYERS: n_z * cells, the states of one block
    int n_z, step_z;                // LAYERS: the layers, and the largest power of two <= n_z + 1
};

// the ordered key of a float32: a total order -inf < ... < -0.0 < +0.0 < ... < +inf; 0 and 0xFFFFFFFF are keys of NaNs alone
__device__ __forceinline__ unsigned comp_key(float f)
{
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float comp_unkey(unsigned k)
{
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// A workgroup owns one stretch of COMP_STRETCH consecutive gates of ONE block and ONE field (a launch per requested field) and
// never crosses a block boundary; the edges of both axes lie in LDS.  Per gate: two branch-free binary searches, the slab test,
// the keys.  Consecutive gates of a ray fall into the same or neighbouring cells, so with COMBINE the lanes of a wavefront that
// form a run of one cell are combined first (a segmented max / min over __shfl_up, bounded by the run's first lane: exact, max
// and min being associative and commutative, and the count of a run is its length), and only the LAST lane of each run issues
// the global integer atomics.  Without COMBINE every counting lane issues its own.
// GATES: the gate plane (CPOL_COMP_PLANE_GATES) -- x and y are two float64 loads per gate, gx[gg] and gy[gg], in place of `dist`
// and the wave-uniform sine / cosine pair; no multiplication, and a NaN coordinate does not count.  Everything behind the
// coordinates is the same code: consecutive gates of a ray still fall into the same or neighbouring cells on any sensible plane.
// LAYERS: height layers (cpol_composite.n_z) -- the float32 layer edges lie in LDS behind the x and y edges, a third branch-free
// search gives iz (comparisons in float32 alone: the slab test of the plain form is not compiled), and the cell index becomes
// iz * cells + iy * n_x + ix within a block of n_z * cells.  The in-wavefront combine is the same code on that index: its runs
// are runs of equal (layer, cell) -- long at a low elevation, a few gates at a steep one, where a ray changes layer every few
// gates.  MAX and the count alone (comp_check refuses the other products with layers), so want_low and n_thr are off by the
// arguments.  LAYERS = false is the kernel as it was.
template <bool COMBINE, bool GATES, bool LAYERS = false>
__global__ __launch_bounds__(COMP_THREADS) void k_comp(const CompArgs a)
{
    extern __shared__ double comp_lds[];
    const int tid = threadIdx.x;
    double *const ex = comp_lds, *const ey = comp_lds + a.n_ex;
    float *const ez = (float *)(comp_lds + a.n_ex + a.n_ey);
    for (int j = tid; j < a.n_ex; j += COMP_THREADS) ex[j] = a.ex[j];
    for (int j = tid; j < a.n_ey; j += COMP_THREADS) ey[j] = a.ey[j];
    if (LAYERS)
        for (int j = tid; j <= a.n_z; j += COMP_THREADS) ez[j] = a.ez[j];
    __syncthreads();
    const long b = (long)blockIdx.x / a.stretches;
    const long s = (long)blockIdx.x % a.stretches;
    const long g0 = b * a.block_gates + s * (long)COMP_STRETCH;
    const long g1 = min(g0 + (long)COMP_STRETCH, (b + 1) * a.block_gates);
    const bool want_max = a.smax != nullptr, want_low = a.slow != nullptr;
    const long cell0 = LAYERS ? b * a.block_cells : b * (long)a.cells;
    // (every lane of the workgroup takes every turn of the loop: the shuffles below need whole wavefronts)
    for (long base = g0; base < g1; base += COMP_THREADS) {
        const long g = base + tid;
        int cell = -1;
        unsigned long long kmax = 0ull, klow = ~0ull;
        unsigned top[COMP_MAX_THR] = {0u, 0u, 0u, 0u};
        if (g < g1) {
            const float v = a.v[g];
            const long gg = g < a.geo_gates ? g : g % a.geo_gates;      // (the geometry of an ensemble call: n_rays rows once)
            const float h = a.hgt[gg];
            double x, y;
            bool located;
            if (GATES) {
                x = a.gx[gg]; y = a.gy[gg];
                located = x == x && y == y;
            } else {
                const int ray = (int)(gg / a.n_gates);
                const float d = a.dist[gg];
                x = (double)d * a.ray_sin[ray]; y = (double)d * a.ray_cos[ray];
                located = d == d;
            }
            const int ix = hist_bin<double>(ex, a.n_ex, a.step_x, x) - 1;
            const int iy = hist_bin<double>(ey, a.n_ey, a.step_y, y) - 1;
            bool counts = v == v && located && h == h && ix >= 0 && ix < a.n_x && iy >= 0 && iy < a.n_y;
            int iz = 0;
            if (LAYERS) {
                // (h NaN: no edge <= h, iz = -1; h on the last edge or above: iz = n_z)
                iz = hist_bin<float>(ez, a.n_z + 1, a.step_z, h) - 1;
                counts = counts && iz >= 0 && iz < a.n_z;
            } else if (a.slab) counts = counts && a.h_lo <= h && h < a.h_hi;
            if (counts) {
                cell = LAYERS ? iz * a.cells + iy * a.n_x + ix : iy * a.n_x + ix;
                const unsigned kv = comp_key(v), kh = comp_key(h);
                kmax = ((unsigned long long)kv << 32) | kh;
                klow = ((unsigned long long)kh << 32) | kv;
#pragma unroll
                for (int j = 0; j < COMP_MAX_THR; ++j) top[j] = (j < a.n_thr && v >= a.thr[j]) ? kh : 0u;
            }
        }
        unsigned long long n = 1ull;
        bool issue = cell >= 0;
        if (COMBINE) {
            const int lane = tid & 63;
            const int before = __shfl_up(cell, 1);
            const bool head = lane == 0 || before != cell || cell < 0;                    // (a gate that does not count: a run of its own)
            const unsigned long long heads = __ballot(head) & (~0ull >> (63 - lane));     // the heads at or below this lane
            const int run = lane - (63 - __clzll((long long)heads));                       // lanes of this run before this one
            for (int dlt = 1; dlt < 64 && __any(run >= dlt); dlt <<= 1) {
                const bool take = run >= dlt;
                if (want_max) { const unsigned long long o = __shfl_up(kmax, dlt); if (take && o > kmax) kmax = o; }
                if (want_low) { const unsigned long long o = __shfl_up(klow, dlt); if (take && o < klow) klow = o; }
#pragma unroll
                for (int j = 0; j < COMP_MAX_THR; ++j)
                    if (j < a.n_thr) { const unsigned o = __shfl_up(top[j], dlt); if (take && o > top[j]) top[j] = o; }
            }
            const int after = __shfl_down(cell, 1);
            issue = issue && (lane == 63 || after != cell);
            n = (unsigned long long)(run + 1);
        }
        if (issue) {
            const long c = cell0 + cell;
            atomicAdd(&a.scount[c], n);
            if (want_max) atomicMax(&a.smax[c], kmax);
            if (want_low) atomicMin(&a.slow[c], klow);
#pragma unroll
            for (int j = 0; j < COMP_MAX_THR; ++j)
                if (j < a.n_thr && top[j]) atomicMax(&a.stop[(b * a.n_thr + j) * (long)a.cells + cell], top[j]);
        }
    }
}

// ---- SOURCE (CPOL_COMP_SOURCE): which call supplied each cell ----
struct CompMergeArgs {
    unsigned long long *rmax, *rlow, *rcount;         // the running state of this field, as in CompArgs (NULL: not requested)
    unsigned *rtop;
    unsigned long long *smax, *slow, *scount;         // the scratch state the call's k_comp filled: the same layout
    unsigned *stop;
    unsigned char *bmax, *blow;     // the source bytes of the running MAX and LOWEST states [n_blocks][cells]
    long n;                         // n_blocks * cells
    int cells, n_thr;
    unsigned source;                // of this call, 0 ... 254
};

// One pass of integer atomics cannot know the final state, so a call of a SOURCE pass composes into a scratch state of its own
// (k_comp, unchanged) and this kernel folds it into the running state: one thread per (block, cell) of one field, ordered behind
// k_comp by the stream, so plain loads and stores do.  A scratch state greater than the running MAX state takes the cell and
// its source byte; an equal one that is not empty lowers the byte to the smaller source (LOWEST mirrored); counts add, echo
// tops take the maximum.  The final byte is the smallest source among the calls that reached the final state, whatever their
// order.  Every scratch word touched goes back to its begin value: no memset runs per call.
__global__ __launch_bounds__(COMP_THREADS) void k_comp_merge(const CompMergeArgs a)
{
    const long i = (long)blockIdx.x * COMP_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const unsigned long long n = a.scount[i];
    if (n == 0ull) return;          // (no gate of this call counted here: every scratch word of the cell holds its begin value)
    a.rcount[i] += n;
    a.scount[i] = 0ull;
    const unsigned char src = (unsigned char)a.source;
    if (a.smax) {
        const unsigned long long s = a.smax[i], r = a.rmax[i];
        if (s > r) { a.rmax[i] = s; a.bmax[i] = src; }
        else if (s == r && src < a.bmax[i]) a.bmax[i] = src;
        a.smax[i] = 0ull;
    }
    if (a.slow) {
        const unsigned long long s = a.slow[i], r = a.rlow[i];
        if (s < r) { a.rlow[i] = s; a.blow[i] = src; }
        else if (s == r && src < a.blow[i]) a.blow[i] = src;
        a.slow[i] = ~0ull;
    }
    const long b = i / a.cells, c = i % a.cells;
    for (int j = 0; j < a.n_thr; ++j) {
        const long at = (b * a.n_thr + j) * (long)a.cells + c;
        const unsigned s = a.stop[at];
        if (s > a.rtop[at]) a.rtop[at] = s;
        if (s) a.stop[at] = 0u;
    }
}

struct CompFinishArgs {
    const unsigned long long *smax, *slow, *scount;   // as in CompArgs
    const unsigned *stop;
    float *values;                  // [n_blocks][n_planes][cells]
    unsigned long long *count;      // [n_blocks][n_fields][cells], at this field's row of block 0
    long n;                         // n_blocks * cells
    int cells, n_planes, n_fields, n_thr;
    const unsigned char *bmax, *blow;   // SOURCE: the source bytes (NULL: no source_of_* planes)
};

// A finishing call: one thread per (block, cell) of one field decodes the states into the planes of `values` -- the key
// inverted, a cell whose state still holds the begin value NaN -- and copies the count.
__global__ __launch_bounds__(COMP_THREADS) void k_comp_finish(const CompFinishArgs a)
{
    const long i = (long)blockIdx.x * COMP_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const long b = i / a.cells, c = i % a.cells;
    const float nan = __uint_as_float(0x7FC00000u);
    float *out = a.values + b * (long)a.n_planes * a.cells + c;
    if (a.smax) {
        const unsigned long long s = a.smax[i];
        out[0] = s ? comp_unkey((unsigned)(s >> 32)) : nan;
        out[a.cells] = s ? comp_unkey((unsigned)s) : nan;
        out += 2 * (long)a.cells;
        if (a.bmax) { out[0] = s ? (float)a.bmax[i] : nan; out += a.cells; }
    }
    if (a.slow) {
        const unsigned long long s = a.slow[i];
        out[0] = s != ~0ull ? comp_unkey((unsigned)s) : nan;
        out[a.cells] = s != ~0ull ? comp_unkey((unsigned)(s >> 32)) : nan;
        out += 2 * (long)a.cells;
        if (a.blow) { out[0] = s != ~0ull ? (float)a.blow[i] : nan; out += a.cells; }
    }
    for (int j = 0; j < a.n_thr; ++j) {
        const unsigned s = a.stop[(b * a.n_thr + j) * (long)a.cells + c];
        out[(long)j * a.cells] = s ? comp_unkey(s) : nan;
    }
    a.count[b * (long)a.n_fields * a.cells + c] = a.scount[i];
}

// ---- the column of the height layers (CPOL_COMP_COLUMN): VIL and its kin ----
struct CompColumnArgs {
    const unsigned long long *smax; // this field's MAX states [n_blocks][n_z][cells]
    const double *tf;               // the table's values [n_tab] ...
    const float *tv;                // ... and breakpoints [n_tab], on the device
    const float *ez;                // the rounded layer edges [n_z + 1]
    double *column;                 // [n_blocks][cells]
    unsigned char *layers;          // [n_blocks][cells]
    long n;                         // n_blocks * cells
    int cells, n_z, n_tab;
    int step_t;                     // the largest power of two <= n_tab
    int gaps;                       // CPOL_COMP_GAPS_ZERO / CPOL_COMP_GAPS_HOLD
};

// One thread per (block, cell) of one field; the field's table (at most 4 KB of breakpoints and 8 KB of values) and the layer
// edges lie in LDS.  The thread walks its cell's layers in ascending order -- stride `cells`, so the loads of a wavefront
// coalesce -- and per counting layer decodes the key, searches the table (comparisons in float32 alone), interpolates with
// separately rounded float64 operations (-ffp-contract=off) and adds f * dz to the running float64 sum: at most 64 terms in a
// fixed order, so the sum is composite.column_of's bit for bit.  HOLD: an empty layer below the highest counting layer (found
// by a first short loop over the states) and above the lowest repeats the f of the nearest counting layer below.  No atomics.
__global__ __launch_bounds__(COMP_THREADS) void k_comp_column(const CompColumnArgs a)
{
    __shared__ double tf[COMP_MAX_TABLE];
    __shared__ float tv[COMP_MAX_TABLE];
    __shared__ float ez[COMP_MAX_LAYERS + 1];
    for (int j = threadIdx.x; j < a.n_tab; j += COMP_THREADS) { tf[j] = a.tf[j]; tv[j] = a.tv[j]; }
    for (int j = threadIdx.x; j <= a.n_z; j += COMP_THREADS) ez[j] = a.ez[j];
    __syncthreads();
    const long i = (long)blockIdx.x * COMP_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const long b = i / a.cells, c = i % a.cells;
    const unsigned long long *const s = a.smax + b * (long)a.n_z * a.cells + c;
    int top = -1;                   // the highest counting layer
    if (a.gaps == CPOL_COMP_GAPS_HOLD)
        for (int l = 0; l < a.n_z; ++l)
            if (s[(long)l * a.cells]) top = l;
    double sum = 0.0, held = 0.0;
    int used = 0;
    bool seen = false;              // a counting layer lies below
    for (int l = 0; l < a.n_z; ++l) {
        const unsigned long long st = s[(long)l * a.cells];
        const bool have = st != 0ull;
        if (have) {
            const float v = comp_unkey((unsigned)(st >> 32));
            const int j = hist_bin<float>(tv, a.n_tab, a.step_t, v) - 1;
            if (j < 0) held = 0.0;
            else if (j >= a.n_tab - 1) held = tf[a.n_tab - 1];
            else {
                const double t = ((double)v - (double)tv[j]) / ((double)tv[j + 1] - (double)tv[j]);
                const double d = tf[j + 1] - tf[j];
                const double p = t * d;
                held = tf[j] + p;
            }
        }
        const bool adds = have || (seen && l < top);
        seen = seen || have;
        if (adds) {
            const double dz = (double)ez[l + 1] - (double)ez[l];
            const double term = held * dz;
            sum = sum + term;
            ++used;
        }
    }
    a.column[i] = seen ? sum : __longlong_as_double(0x7FF8000000000000ll);
    a.layers[i] = (unsigned char)used;
}

// ---- the exact sums (CPOL_COMP_SUM, cpol_composite_sums): the cell mean, rain accumulations ----
struct CompSumArgs {
    CompArgs a;                     // as k_comp takes them (the states of k_comp are not read: smax, slow, scount, stop stay NULL)
    const double *wf;               // the weight table's values [n_w] ...
    const float *wv;                // ... and breakpoints [n_w], on the device (n_w == 0: w = v)
    int n_w, step_w;                // step_w: the largest power of two <= n_w
    unsigned long long *bins;       // this field's rows [n_blocks * block_cells][COMP_SUM_BINS], int64 as two's complement
    unsigned *skipped;              // [n_blocks * block_cells]
};

// One launch per requested field behind that field's k_comp, with k_comp's ownership: a workgroup owns one stretch of COMP_STRETCH
// consecutive gates of ONE block and never crosses a block boundary; the edges lie in LDS as in k_comp, the weight table behind
// them (at most 8 KB of values and 4 KB of breakpoints), the layer edges last.  The cell of a gate: k_comp's statements.  Per
// counting gate the weight w (obj_weight, or v itself), its split into sign, E and M (obj_sum_split), the term +-M << (E & 7)
// (obj_sum_term, below 2^31) and the key (cell, E >> 3): the bin of the state the term goes to.  Consecutive gates of a ray share
// the cell and nearly always the exponent bin, so with COMBINE the lanes of a wavefront that form a run of equal key are summed
// first (a segmented INTEGER sum over __shfl_up, bounded by the run's first lane: at most 64 terms below 2^31, below 2^37, no
// overflow; integer addition is associative and commutative, so the sum is exact whatever the grouping), and the LAST lane of
// each run issues ONE 64-bit integer atomicAdd.  Without COMBINE every summed lane issues its own.  A gate whose w is not
// finite adds one to the cell's skipped word (rare).  No float atomics, no compare-and-swap loops; the loop bounds: COMP_STRETCH /
// COMP_THREADS turns, 6 steps of the scan, 11 of a search.  Every lane of the workgroup takes every turn of the gate loop.
template <bool COMBINE, bool GATES, bool LAYERS>
__global__ __launch_bounds__(COMP_THREADS) void k_comp_sum(const CompSumArgs s)
{
    extern __shared__ double comp_lds[];
    const CompArgs &a = s.a;
    const int tid = threadIdx.x;
    double *const ex = comp_lds, *const ey = ex + a.n_ex, *const wf = ey + a.n_ey;
    float *const wv = (float *)(wf + s.n_w), *const ez = wv + s.n_w;
    for (int j = tid; j < a.n_ex; j += COMP_THREADS) ex[j] = a.ex[j];
    for (int j = tid; j < a.n_ey; j += COMP_THREADS) ey[j] = a.ey[j];
    for (int j = tid; j < s.n_w; j += COMP_THREADS) { wf[j] = s.wf[j]; wv[j] = s.wv[j]; }
    if (LAYERS)
        for (int j = tid; j <= a.n_z; j += COMP_THREADS) ez[j] = a.ez[j];
    __syncthreads();
    const long b = (long)blockIdx.x / a.stretches;
    const long st = (long)blockIdx.x % a.stretches;
    const long g0 = b * a.block_gates + st * (long)COMP_STRETCH;
    const long g1 = min(g0 + (long)COMP_STRETCH, (b + 1) * a.block_gates);
    const long cell0 = LAYERS ? b * a.block_cells : b * (long)a.cells;
    // (every lane of the workgroup takes every turn of the loop: the shuffles below need whole wavefronts)
    for (long base = g0; base < g1; base += COMP_THREADS) {
        const long g = base + tid;
        int cell = -1, key = -1;      // key: (cell, bin) of a summed gate
        long long term = 0ll;
        bool skip = false;
        if (g < g1) {
            const float v = a.v[g];
            const long gg = g < a.geo_gates ? g : g % a.geo_gates;      // (the geometry of an ensemble call: n_rays rows once)
            const float h = a.hgt[gg];
            double x, y;
            bool located;
            if (GATES) {
                x = a.gx[gg]; y = a.gy[gg];
                located = x == x && y == y;
            } else {
                const int ray = (int)(gg / a.n_gates);
                const float d = a.dist[gg];
                x = (double)d * a.ray_sin[ray]; y = (double)d * a.ray_cos[ray];
                located = d == d;
            }
            const int ix = hist_bin<double>(ex, a.n_ex, a.step_x, x) - 1;
            const int iy = hist_bin<double>(ey, a.n_ey, a.step_y, y) - 1;
            bool counts = v == v && located && h == h && ix >= 0 && ix < a.n_x && iy >= 0 && iy < a.n_y;
            int iz = 0;
            if (LAYERS) {
                iz = hist_bin<float>(ez, a.n_z + 1, a.step_z, h) - 1;
                counts = counts && iz >= 0 && iz < a.n_z;
            } else if (a.slab) counts = counts && a.h_lo <= h && h < a.h_hi;
            if (counts) {
                cell = LAYERS ? iz * a.cells + iy * a.n_x + ix : iy * a.n_x + ix;
                const float w = s.n_w ? obj_weight(wv, wf, s.n_w, s.step_w, v) : v;
                const unsigned bits = __float_as_uint(w);
                int E;
                unsigned M;
                if (obj_sum_split(bits, &E, &M)) {
                    term = obj_sum_term(bits, M, 1u, E & 7);
                    key = cell * COMP_SUM_BINS + (E >> 3);            // (cell < 2^26: below 2^31)
                } else skip = true;
            }
        }
        bool issue = key >= 0;
        if (COMBINE) {
            const int lane = tid & 63;
            const int before = __shfl_up(key, 1);
            const bool head = lane == 0 || before != key || key < 0;                      // (a gate that is not summed: a run of its own)
            const unsigned long long heads = __ballot(head) & (~0ull >> (63 - lane));     // the heads at or below this lane
            const int run = lane - (63 - __clzll((long long)heads));                       // lanes of this run before this one
            for (int dlt = 1; dlt < 64 && __any(run >= dlt); dlt <<= 1) {
                const long long o = __shfl_up(term, dlt);
                if (run >= dlt) term += o;
            }
            const int after = __shfl_down(key, 1);
            issue = issue && (lane == 63 || after != key);
        }
        if (issue) atomicAdd(&s.bins[(cell0 + cell) * (long)COMP_SUM_BINS + (key & (COMP_SUM_BINS - 1))], (unsigned long long)term);
        if (skip) atomicAdd(&s.skipped[cell0 + cell], 1u);
    }
}

struct CompSumFinishArgs {
    const unsigned long long *bins;     // as in CompSumArgs
    const unsigned *skipped;
    const unsigned long long *scount;   // this field's counts, as in CompArgs
    double *sum;                        // [n_blocks][n_z or absent][cells]
    unsigned *sum_skipped;              // likewise
    long n;                             // n_blocks * block_cells
};

// A finishing call: one thread per (block, layer, cell) of one field rounds the cell's row once (obj_sum_round: the bins
// propagated into one integer, its top 53 bits, ties to even; +0.0 for an exact zero), writes NaN where no gate was summed
// (count - skipped == 0) and copies the skipped word.
__global__ __launch_bounds__(COMP_THREADS) void k_comp_sum_finish(const CompSumFinishArgs a)
{
    const long i = (long)blockIdx.x * COMP_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const unsigned sk = a.skipped[i];
    const unsigned long long n = a.scount[i];
    const unsigned long long r = n - (unsigned long long)sk ? obj_sum_round(a.bins + i * (long)COMP_SUM_BINS, COMP_SUM_BINS, 8) : 0x7FF8000000000000ull;
    a.sum[i] = __longlong_as_double((long long)r);
    a.sum_skipped[i] = sk;
}
