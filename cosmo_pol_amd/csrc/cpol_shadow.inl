// cpol_shadow.inl -- terrain shadowing: a sub-beam stays blocked behind its first gate below the topography, and the visible
// share of the antenna pattern per gate.  include/cosmo_pol_amd.h ("Terrain shadowing") and cosmo_pol_amd/shadow.py state the rule.
//
// Reference functions replaced (wolfidan/cosmo_pol): nothing that runs.  interpolation_c.c:92-102 writes NaN (or -9999) into every
// gate from the hit onward ("We hit a mountain") and its own loop overwrites those gates on later iterations, so every gate of the
// reference depends on itself alone -- what the gate kernels restate and what stays the default.  k_terrain_shadow is the
// fill-forward the reference meant, as a step of its own between the interpolation and everything that reads the columns.
//
// LAYOUT: mask[row][gate] with row = (ray, sub-beam) -- in an ensemble call (member, ray, sub-beam), cpol_members.inl -- and
// vals[v][row][gate]: the work arrays b_mask / b_vals as every interpolating form leaves them.  Every form writes the code of
// every gate of its launch afresh (k_interp_sweep / record / replay: a.mask[sbg] on each of their three exits; the member forms:
// members_fill / members_values' finish), the replay form from the recorded class and the values it has just interpolated, never
// from b_mask -- so the kernel always sees unshadowed codes, and running it twice changes nothing either (it is idempotent).

#ifndef CPOL_SHADOW_THREADS
#define CPOL_SHADOW_THREADS 256       // 4 wavefronts = 4 rows per workgroup
#endif

// One wavefront per row.  The row is walked in chunks of 64 gates, gates on lanes: the first chunk with a code -1 gives `first`
// (ballot, lowest set bit); from there on every gate's code becomes -1 and its n_vars values NaN, whatever they were -- 64
// consecutive bytes / floats per store instruction.  Both loops are bounded by ceil(n_gates / 64); no atomics, no LDS, no
// communication between wavefronts.
__global__ __launch_bounds__(CPOL_SHADOW_THREADS) void k_terrain_shadow(signed char *__restrict__ mask, float *__restrict__ vals,
                                                                       long n_rows, int n_gates, int n_vars)
{
    const int lane = (int)(threadIdx.x & 63);
    const long row = (long)blockIdx.x * (CPOL_SHADOW_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;                              // (wave-uniform)
    const long at = row * n_gates, plane = n_rows * n_gates;
    const int n_chunks = (n_gates + 63) / 64;
    int first = n_gates;
    for (int c = 0; c < n_chunks; ++c) {
        const int g = c * 64 + lane;
        const bool hit = g < n_gates && mask[at + g] == -1;
        const unsigned long long b = __builtin_amdgcn_ballot_w64(hit);
        if (b) { first = c * 64 + __builtin_ctzll(b); break; }     // (wave-uniform)
    }
    if (first >= n_gates) return;
    const float qnan = __builtin_nanf("");                  // the NaN of the gate kernels' masked gates
    for (int c = first / 64; c < n_chunks; ++c) {
        const int g = c * 64 + lane;
        if (g < first || g >= n_gates) continue;
        mask[at + g] = -1;
        for (int v = 0; v < n_vars; ++v) vals[(long)v * plane + at + g] = qnan;
    }
}

// One thread per (ray, gate): the weights of the sub-beams whose code is not -1, summed ascending in float64 from +0.0, over the
// sum of all weights (FinalArgs::sum_w, formed the same way on the host).  The TU is built with -ffp-contract=off.
__global__ __launch_bounds__(256) void k_visibility(const signed char *__restrict__ mask, const double *__restrict__ sub_w,
                                                    double *__restrict__ vis, long n_rg, int n_gates, int n_sub, double sum_w)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rg) return;
    const long ray = i / n_gates;
    const int gate = (int)(i - ray * n_gates);
    double s_w = 0.0;
    for (int s = 0; s < n_sub; ++s)
        if (mask[(ray * n_sub + s) * n_gates + gate] != -1) s_w += sub_w[s];
    vis[i] = s_w / sum_w;
}
