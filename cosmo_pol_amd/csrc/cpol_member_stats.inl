// cpol_member_stats.inl -- ensemble statistics: the members of a pass folded, one after another, into a running state per gate
// (cpol_member_stats): mean, spread, extremes, the members that count and the members above thresholds; and, for the fields
// that ask for them, quantiles of the members (k_member_quantile: the fold stashes the members, a finishing call sorts each
// cell's counting members in LDS and reads the order statistics).
//
// k_member_verify scores the same members against an observation per cell (cpol_member_verify): the observation's rank among them
// and the CRPS, read off the column sorted once more.
//
// Reference functions replaced (wolfidan/cosmo_pol): none -- the reference runs one model state per process.  The rule is the
// one of include/cosmo_pol_amd.h and cosmo_pol_amd/ensemble_stats.py (`fold`, `finish`), ORDER-EXACT: a strict left fold over
// the members (Welford's update: one float64 subtraction, division, addition, subtraction, multiplication, addition per
// counting value), then one float64 division, square root and rounding.  Only IEEE operations, and the TU is compiled with
// -ffp-contract=off -fno-fast-math: the kernels give the bits of the NumPy statement however the pass is cut into calls.
// The division by n is part of the rule: no reciprocal.

#define CPOL_MS_FIELDS 10           // ZH, ZV, ZDR, KDP, DELTA_HV, PHIDP, RHOHV, ATT_H, ATT_V, RVEL (the rows of `count`)
#define CPOL_MS_RVEL 9
#define CPOL_MS_MAX_THR 8
#define CPOL_MS_MAX_Q 8
#define CPOL_MS_MAX_Q_MEMBERS 128

// the running state of one folded field, SoA: the lanes of a wavefront touch consecutive addresses of every array
struct MemberState {
    unsigned short *n;              // [n_cells]
    double *mean, *m2;              // [n_cells]
    void *lo, *hi;                  // [n_cells] of the field's type
    unsigned short *k;              // [n_thr][n_cells]
};

struct MemberStatsArgs {
    const void *in[CPOL_MS_FIELDS];         // per-gate fields, row set m at element m * n_cells (float32; slot RVEL float64)
    MemberState st[CPOL_MS_FIELDS];
    double thr[CPOL_MS_FIELDS][CPOL_MS_MAX_THR];    // float32 fields: already rounded to float32
    int n_thr[CPOL_MS_FIELDS];
    int field[CPOL_MS_FIELDS];              // the folded fields = gridDim.y
    int n_fields;
    int n_sets;                             // row sets (members) of this call
    int begin;                              // 1: the state starts here (nothing is loaded)
    int need;                               // min_members
    long n_cells;
    // k_member_finish
    void *o_mean[CPOL_MS_FIELDS], *o_spread[CPOL_MS_FIELDS], *o_min[CPOL_MS_FIELDS], *o_max[CPOL_MS_FIELDS];
    unsigned short *o_count;                // [10][n_cells] or NULL
    unsigned short *o_exceed[CPOL_MS_FIELDS];
    int zero_rest;                          // 1: the rows of `count` of fields not folded are written as zeros
    // quantiles: where k_member_fold keeps the members of a field with quantiles ([capacity][n_cells] of the field's type; NULL:
    // the field has none), and the row of this call's first member
    void *stash[CPOL_MS_FIELDS];
    int row0;
};

struct MemberQuantileArgs {
    const void *stash[CPOL_MS_FIELDS];      // [members][n_cells] of the field's type, rows in fold order
    void *out[CPOL_MS_FIELDS];              // [n_q][n_cells] of the field's type
    double q[CPOL_MS_FIELDS][CPOL_MS_MAX_Q];
    int n_q[CPOL_MS_FIELDS];
    int field[CPOL_MS_FIELDS];              // the fields with quantiles whose output is wanted = gridDim.y
    int members;                            // rows of the stash that hold a member (<= 128): the LDS column's height
    int method;                             // 0 linear, 1 lower, 2 higher, 3 nearest
    int need;
    long n_cells;
};

struct MemberVerifyArgs {
    const void *stash[CPOL_MS_FIELDS];      // [members][n_cells] of the field's type, rows in fold order
    const void *obs[CPOL_MS_FIELDS];        // [n_cells] of the field's type; NaN: no observation
    unsigned short *below[CPOL_MS_FIELDS], *equal[CPOL_MS_FIELDS];      // [n_cells] or NULL
    void *crps[CPOL_MS_FIELDS];             // [n_cells] of the field's type or NULL
    int field[CPOL_MS_FIELDS];              // the verified fields whose output is wanted = gridDim.y
    int members;                            // rows of the stash that hold a member (<= 128): the LDS column's height
    int fair;                               // 1: the pair term is divided by n (n - 1)
    int need;
    long n_cells;
};

// x / n (n a whole number, 1 <= n <= 65535) rounded ONCE, whatever the quotient.  The device's float64 division is correctly
// rounded for a normal quotient; a SUBNORMAL one can come out one unit of the subnormal grid off (measured: 4 of 160 000 means
// of 1e-310-sized members, always away from the CPU's division by one unit).  The residual x - q n of such a quotient is a small
// multiple of 2^-1074, so the fma gives it exactly, and it says which neighbour of q is the nearest (ties to even).
__device__ __forceinline__ double member_div(double x, double n)
{
    double q = x / n;
    if (__builtin_fabs(q) < 2.2250738585072014e-308) {       // (false for NaN)
        const double ulp = 4.9406564584124654e-324;
        const double r = __builtin_fma(-q, n, x);
        const double r2 = r + r, nu = n * ulp;
        const bool odd = (__double_as_longlong(q) & 1) != 0;
        if (r2 > nu || (r2 == nu && odd)) q = q + ulp;
        else if (r2 < -nu || (r2 == -nu && odd)) q = q - ulp;
    }
    return q;
}

template <typename T>
__device__ __forceinline__ void member_fold_field(const MemberStatsArgs &a, int f, long c)
{
    const MemberState &s = a.st[f];
    const int n_thr = a.n_thr[f];
    unsigned n = 0;
    double mean = 0.0, m2 = 0.0;
    T lo = (T)__builtin_inf(), hi = (T)-__builtin_inf();
    unsigned k[CPOL_MS_MAX_THR];
    T thr[CPOL_MS_MAX_THR];
#pragma unroll
    for (int t = 0; t < CPOL_MS_MAX_THR; ++t) { k[t] = 0; thr[t] = (T)a.thr[f][t]; }
    if (!a.begin) {
        n = s.n[c]; mean = s.mean[c]; m2 = s.m2[c];
        lo = ((const T *)s.lo)[c]; hi = ((const T *)s.hi)[c];
#pragma unroll
        for (int t = 0; t < CPOL_MS_MAX_THR; ++t)
            if (t < n_thr) k[t] = s.k[(long)t * a.n_cells + c];
    }
    const T *__restrict__ x = (const T *)a.in[f];
    T *const stash = (T *)a.stash[f];         // (wave-uniform: a pass without quantiles runs what it ran without them)
    for (int m = 0; m < a.n_sets; ++m) {
        const T v = x[(long)m * a.n_cells + c];
        if (stash) stash[(long)(a.row0 + m) * a.n_cells + c] = v;
        if (v == v) {
            n = n + 1;
            const double d = (double)v - mean;
            mean = mean + member_div(d, (double)n);
            m2 = m2 + d * ((double)v - mean);
            if (v < lo) lo = v;
            if (v > hi) hi = v;
#pragma unroll
            for (int t = 0; t < CPOL_MS_MAX_THR; ++t)
                if (t < n_thr) k[t] += v > thr[t];
        }
    }
    s.n[c] = (unsigned short)n; s.mean[c] = mean; s.m2[c] = m2;
    ((T *)s.lo)[c] = lo; ((T *)s.hi)[c] = hi;
#pragma unroll
    for (int t = 0; t < CPOL_MS_MAX_THR; ++t)
        if (t < n_thr) s.k[(long)t * a.n_cells + c] = (unsigned short)k[t];
}

// One lane per (cell, folded field); the members of the call at stride n_cells; the state is loaded and stored once per call.
__global__ __launch_bounds__(256) void k_member_fold(const MemberStatsArgs a)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n_cells) return;
    const int f = a.field[blockIdx.y];
    if (f == CPOL_MS_RVEL) member_fold_field<double>(a, f, c);
    else member_fold_field<float>(a, f, c);
}

template <typename T>
__device__ __forceinline__ void member_finish_field(const MemberStatsArgs &a, int f, long c)
{
    const MemberState &s = a.st[f];
    const int n = s.n[c];
    const T nan = (T)__builtin_nan("");
    if (a.o_mean[f]) ((T *)a.o_mean[f])[c] = n >= a.need ? (T)s.mean[c] : nan;
    if (a.o_spread[f]) ((T *)a.o_spread[f])[c] = n >= max(a.need, 2) ? (T)__builtin_sqrt(member_div(s.m2[c], (double)(n - 1))) : nan;
    if (a.o_min[f]) ((T *)a.o_min[f])[c] = n >= a.need ? ((const T *)s.lo)[c] : nan;
    if (a.o_max[f]) ((T *)a.o_max[f])[c] = n >= a.need ? ((const T *)s.hi)[c] : nan;
    if (a.o_count) a.o_count[(long)f * a.n_cells + c] = (unsigned short)n;
    if (a.o_exceed[f])
        for (int t = 0; t < a.n_thr[f]; ++t) a.o_exceed[f][(long)t * a.n_cells + c] = s.k[(long)t * a.n_cells + c];
}

__global__ __launch_bounds__(256) void k_member_finish(const MemberStatsArgs a)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n_cells) return;
    const int f = a.field[blockIdx.y];
    if (f == CPOL_MS_RVEL) member_finish_field<double>(a, f, c);
    else member_finish_field<float>(a, f, c);
    if (a.o_count && a.zero_rest && blockIdx.y == 0) {
        unsigned folded = 0;
        for (int j = 0; j < a.n_fields; ++j) folded |= 1u << a.field[j];
        for (int j = 0; j < CPOL_MS_FIELDS; ++j)
            if (!((folded >> j) & 1u)) a.o_count[(long)j * a.n_cells + c] = 0;
    }
}

// ---- quantiles ----
// The rule's order as an unsigned compare: the bits of a negative value flipped, the sign bit of a non-negative one set
// (-0.0 before +0.0, -inf first, +inf last; NaNs never get here).
__device__ __forceinline__ unsigned member_key(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u >> 31) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ unsigned long long member_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ float member_unkey(unsigned k) { return __uint_as_float((k >> 31) ? k & 0x7fffffffu : ~k); }
__device__ __forceinline__ double member_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

// One lane per cell; the lane's counting members as keys, sorted by insertion, in its own LDS column col[j * 64] (layout
// [member][lane]: the lanes of a wavefront touch consecutive words, a lane's column walks at stride 64 words).  No lane reads
// another lane's column: no barrier.
template <typename T, typename K>
__device__ __forceinline__ void member_quantile_field(const MemberQuantileArgs &a, int f, long c, K *__restrict__ col)
{
    const T *__restrict__ x = (const T *)a.stash[f];
    int n = 0;
    for (int m = 0; m < a.members; ++m) {
        const T v = x[(long)m * a.n_cells + c];
        if (v == v) {
            const K key = member_key(v);
            int j = n;
            while (j > 0) {
                const K prev = col[(j - 1) * 64];
                if (!(key < prev)) break;
                col[j * 64] = prev;
                --j;
            }
            col[j * 64] = key;
            ++n;
        }
    }
    T *__restrict__ out = (T *)a.out[f];
    const int n_q = a.n_q[f];
    for (int t = 0; t < n_q; ++t) {
        T r = (T)__builtin_nan("");
        if (n >= a.need && n > 0) {
            const double h = a.q[f][t] * (double)(n - 1);       // 0 <= h <= n - 1
            int i = (int)h;                                     // floor
            if (a.method == 0) {
                const double g = h - (double)i;
                const T xa = member_unkey(col[i * 64]);
                r = xa;
                if (g != 0.0) {                                 // (then i + 1 <= n - 1)
                    const T xb = member_unkey(col[(i + 1) * 64]);
                    const double da = (double)xa, db = (double)xb;
                    if (da != db) {
                        const double d = db - da;
                        const double p = g * d;
                        double s = da + p;
                        if (s > db) s = db;
                        r = (T)s;
                    }
                }
            } else {
                if (a.method == 2) i += (double)i < h;
                else if (a.method == 3) i = (int)__builtin_rint(h);
                r = member_unkey(col[i * 64]);
            }
        }
        out[(long)t * a.n_cells + c] = r;
    }
}

// Grid (cells / 64, fields with quantiles); ONE wavefront per workgroup; dynamic LDS: members x 64 keys of the widest field.
__global__ __launch_bounds__(64) void k_member_quantile(const MemberQuantileArgs a)
{
    extern __shared__ unsigned long long member_q_lds[];
    const long c = (long)blockIdx.x * 64 + threadIdx.x;
    if (c >= a.n_cells) return;
    const int f = a.field[blockIdx.y];
    if (f == CPOL_MS_RVEL) member_quantile_field<double, unsigned long long>(a, f, c, member_q_lds + threadIdx.x);
    else member_quantile_field<float, unsigned>(a, f, c, (unsigned *)member_q_lds + threadIdx.x);
}

// ---- verification against observations ----
// One lane per cell, the column of k_member_quantile: the lane's counting members as keys, sorted by insertion, in its own LDS
// column col[j * 64].  One walk counts the keys below and equal to the observation's; one walk forms A = sum |x_i - y| and one
// B = sum (2 i - n + 1) x_i over the sorted values, ascending, in float64.  crps = A / n - B / D, D = n n or n (n - 1), each
// quotient rounded once (member_div), clamped at +0.0.  No lane reads another lane's column: no barrier.
template <typename T, typename K>
__device__ __forceinline__ void member_verify_field(const MemberVerifyArgs &a, int f, long c, K *__restrict__ col)
{
    const T *__restrict__ x = (const T *)a.stash[f];
    int n = 0;
    for (int m = 0; m < a.members; ++m) {
        const T v = x[(long)m * a.n_cells + c];
        if (v == v) {
            const K key = member_key(v);
            int j = n;
            while (j > 0) {
                const K prev = col[(j - 1) * 64];
                if (!(key < prev)) break;
                col[j * 64] = prev;
                --j;
            }
            col[j * 64] = key;
            ++n;
        }
    }
    const T y = ((const T *)a.obs[f])[c];
    const bool seen = y == y;
    if (a.below[f] || a.equal[f]) {
        unsigned below = 0, equal = 0;
        if (seen) {
            const K ky = member_key(y);
            for (int i = 0; i < n; ++i) {
                const K k = col[i * 64];
                below += k < ky;
                equal += k == ky;
            }
        }
        if (a.below[f]) a.below[f][c] = (unsigned short)below;
        if (a.equal[f]) a.equal[f][c] = (unsigned short)equal;
    }
    if (a.crps[f]) {
        T r = (T)__builtin_nan("");
        if (seen && n >= a.need && n > a.fair) {             // (n > 0; fair: n >= 2)
            const double yd = (double)y;
            double A = 0.0, B = 0.0;
            for (int i = 0; i < n; ++i) A = A + __builtin_fabs((double)member_unkey(col[i * 64]) - yd);
            for (int i = 0; i < n; ++i) {
                const double p = (double)(2 * i - n + 1) * (double)member_unkey(col[i * 64]);
                B = B + p;
            }
            const int D = a.fair ? n * (n - 1) : n * n;     // <= 16384
            double s = member_div(A, (double)n) - member_div(B, (double)D);
            if (s < 0.0) s = 0.0;
            r = (T)s;
        }
        ((T *)a.crps[f])[c] = r;
    }
}

// Grid (cells / 64, verified fields whose output is wanted); ONE wavefront per workgroup; dynamic LDS: members x 64 keys of the
// widest field -- the shape of k_member_quantile.
__global__ __launch_bounds__(64) void k_member_verify(const MemberVerifyArgs a)
{
    extern __shared__ unsigned long long member_v_lds[];
    const long c = (long)blockIdx.x * 64 + threadIdx.x;
    if (c >= a.n_cells) return;
    const int f = a.field[blockIdx.y];
    if (f == CPOL_MS_RVEL) member_verify_field<double, unsigned long long>(a, f, c, member_v_lds + threadIdx.x);
    else member_verify_field<float, unsigned>(a, f, c, (unsigned *)member_v_lds + threadIdx.x);
}
