// cpol_superob.inl -- superobservations: the per-gate fields of a call averaged over ray x gate windows (cpol_superob).
//
// Reference functions replaced (wolfidan/cosmo_pol): none -- the reference hands back per-gate radials.  The rule is the
// one of include/cosmo_pol_amd.h and cosmo_pol_amd/superob.py (`average`), ORDER-EXACT: per ray of a window the float64 sum
// of the counting values in ascending gate order from +0.0, then the float64 sum of those in ascending ray order from +0.0,
// one float64 division, one rounding to float32.  Only IEEE adds and one divide, and the TU is compiled with
// -ffp-contract=off -fno-fast-math: the kernel gives the bits of the NumPy statement.  No tree over gates or rays.

#define CPOL_SUPEROB_FIELDS 10      // ZH, ZV, ZDR, KDP, DELTA_HV, PHIDP, RHOHV, ATT_H, ATT_V, RVEL (the rows of `count`)
#define CPOL_SUPEROB_ZV   1
#define CPOL_SUPEROB_ZDR  2
#define CPOL_SUPEROB_RVEL 9

struct SuperobArgs {
    const float *in[CPOL_SUPEROB_FIELDS];   // per-gate float32 fields [n_rows][n_gates] (slot ZDR: unused, slot RVEL: unused)
    const double *in_rvel;                  // per-gate RVEL
    float *out[CPOL_SUPEROB_FIELDS];        // [n_cells] (slot RVEL: unused)
    double *out_rvel;
    unsigned short *count;                  // [10][n_cells] or NULL
    long n_cells;
    double min_valid_fraction;
    int n_gates, R, G, rays_per_block, win_rows, win_cols;    // win_rows / win_cols: windows of one block of rows
    int n_fields;                           // requested fields = gridDim.y
    int field[CPOL_SUPEROB_FIELDS];         // which
    int zero_rest;                          // 1: the rows of `count` nobody asked for are written as zeros
};

// S and n of one field over the window's rays [r0, r1) x gates [g0, g1); `other`: a gate counts only where this is not NaN
// either (ZDR's gate set), or NULL
template <typename T>
__device__ __forceinline__ void superob_sums(const T *__restrict__ x, const float *__restrict__ other, long row0, int r0, int r1,
                                             int g0, int g1, int n_gates, double &S, int &n)
{
    S = 0.0;
    n = 0;
    for (int r = r0; r < r1; ++r) {
        const long base = (row0 + r) * (long)n_gates;
        double s = 0.0;
        for (int g = g0; g < g1; ++g) {
            const T v = x[base + g];
            bool counts = v == v;
            if (other) { const float o = other[base + g]; counts = counts && o == o; }
            if (counts) { s = s + (double)v; ++n; }
        }
        S = S + s;
    }
}

// One lane per (requested field, window); windows column-fastest, so that the lanes of a wavefront walk neighbouring runs of
// G gates of the same rays: over the G steps of the inner loop a wavefront consumes one contiguous stretch of every ray.
__global__ __launch_bounds__(256) void k_superob(const SuperobArgs a)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n_cells) return;
    const int f = a.field[blockIdx.y];
    const int j = (int)(c % a.win_cols);
    const long t = c / a.win_cols;
    const int i = (int)(t % a.win_rows);
    const long row0 = (t / a.win_rows) * (long)a.rays_per_block;
    const int r0 = i * a.R, r1 = min(r0 + a.R, a.rays_per_block);
    const int g0 = j * a.G, g1 = min(g0 + a.G, a.n_gates);
    const int N = (r1 - r0) * (g1 - g0);
    const int need = max(1, (int)ceil(a.min_valid_fraction * (double)N));
    int n;
    if (f == CPOL_SUPEROB_RVEL) {
        double S;
        superob_sums<double>(a.in_rvel, nullptr, row0, r0, r1, g0, g1, a.n_gates, S, n);
        a.out_rvel[c] = n < need ? __builtin_nan("") : S / (double)n;
    } else if (f == CPOL_SUPEROB_ZDR) {
        double SH, SV;
        int nv;
        superob_sums<float>(a.in[0], a.in[CPOL_SUPEROB_ZV], row0, r0, r1, g0, g1, a.n_gates, SH, n);
        superob_sums<float>(a.in[CPOL_SUPEROB_ZV], a.in[0], row0, r0, r1, g0, g1, a.n_gates, SV, nv);
        a.out[f][c] = n < need ? __builtin_nanf("") : (float)(SH / SV);
    } else {
        double S;
        superob_sums<float>(a.in[f], nullptr, row0, r0, r1, g0, g1, a.n_gates, S, n);
        a.out[f][c] = n < need ? __builtin_nanf("") : (float)(S / (double)n);
    }
    if (a.count) {
        a.count[(long)f * a.n_cells + c] = (unsigned short)n;
        if (a.zero_rest && blockIdx.y == 0) {
            unsigned asked = 0;
            for (int k = 0; k < a.n_fields; ++k) asked |= 1u << a.field[k];
            for (int k = 0; k < CPOL_SUPEROB_FIELDS; ++k)
                if (!((asked >> k) & 1u)) a.count[(long)k * a.n_cells + c] = 0;
        }
    }
}
