// cpol_ingest.inl -- model input on the device: GRIB-1 simple packing -> float32 planes -> the staged cube.
//
// Reference functions replaced (wolfidan/cosmo_pol): the pycosmo read of radar_operator.py:217-309
// (open_file / get_variable with assign_heights) as cosmo_pol_amd/model_io.py states it on the host:
//   grib1.decode_values      k_grib_unpack   (the value definition of cosmo_pol_amd/grib1.py, float64, one rounding to float32)
//   model_io.derive, the W / EDR / HHL half-level means of read_model_file, k_stage_heights, k_stage_variable
//                            k_model_derive  (the host statements operand by operand in float64)
// Only IEEE add, multiply, divide and exact scalings, and the TU is compiled with -ffp-contract=off: both kernels give
// the host's bits.

// one packed plane as the kernel sees it
struct PackedPlaneDev {
    unsigned long long off;     // octet offset of the bit string in the arena (a multiple of 16; >= 8 octets of slack behind)
    double ref;                 // R
    double dec;                 // 10 ** |D| (repeated multiplication by 10.0 on the host, as grib1.pow10)
    int bin_scale;              // E
    int dec_sign;               // sign of D
    int n_bits;                 // 0 ... 32
    int flip;                   // rows are stored north to south
    long out_plane;             // plane index in the output cube
};

// packed planes -> float32 planes [out_plane][ny][nx]: one thread per value; lane i reads bit field i, so a wavefront
// reads one contiguous run of octets.  A field of <= 32 bits at a bit offset of <= 31 lies in two aligned big-endian
// words (the arena's slack makes the second one readable behind the last value); X stays unsigned up to 2^32 - 1.
__global__ __launch_bounds__(256) void k_grib_unpack(const unsigned *__restrict__ arena, const PackedPlaneDev *__restrict__ pd,
                                                     float *__restrict__ out, int ny, int nx)
{
    const PackedPlaneDev d = pd[blockIdx.y];
    const long ncell = (long)ny * nx;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ncell) return;
    unsigned x = 0;
    if (d.n_bits) {
        const unsigned *w = arena + (d.off >> 2);
        const unsigned long long bit = (unsigned long long)i * (unsigned)d.n_bits;
        const unsigned long long wi = bit >> 5;
        const unsigned s = (unsigned)(bit & 31);
        const unsigned long long two = ((unsigned long long)__builtin_bswap32(w[wi]) << 32) | __builtin_bswap32(w[wi + 1]);
        x = (unsigned)((two >> (64u - s - (unsigned)d.n_bits)) & (0xFFFFFFFFull >> (32 - d.n_bits)));
    }
    double t = d.ref + ldexp((double)x, d.bin_scale);
    if (d.dec_sign > 0) t = t / d.dec;
    else if (d.dec_sign < 0) t = t * d.dec;
    long o = i;
    if (d.flip) {
        const long row = i / nx;
        o = (long)(ny - 1 - row) * nx + (i - row * nx);
    }
    out[d.out_plane * ncell + o] = (float)t;
}

struct DeriveArgs {
    const float *planes;        // [plane][ny][nx]; plane = base of the raw field + level
    float *V;                   // [cell][nz][n_vars]
    float *H;                   // [cell][nz]
    float2 *HT;                 // [cell] (model top, lowest level)
    long ncell;
    int nz, n_vars, kc, rowlen;
    int base_p, base_t, base_qv, base_hhl, hhl_half;      // hhl_half: HHL on nz + 1 levels (means), else full-level heights (copy)
    int n_load, base_load[CPOL_MAX_LOAD];
    int recipe[CPOL_MAX_VARS], base_src[CPOL_MAX_VARS];
    double r_d, rv_rd_m1;
};

__device__ __forceinline__ float derive_plane(const DeriveArgs &a, int base, int k, long cell)
{
    return a.planes[(long)(base + k) * a.ncell + cell];
}

// float32(0.5 * (float64(x[k]) + x[k + 1]))
__device__ __forceinline__ float derive_half_mean(const DeriveArgs &a, int base, int k, long cell)
{
    return (float)(0.5 * ((double)derive_plane(a, base, k, cell) + (double)derive_plane(a, base, k + 1, cell)));
}

__device__ __forceinline__ float derive_height(const DeriveArgs &a, int k, long cell)
{
    return a.hhl_half ? derive_half_mean(a, a.base_hhl, k, cell) : derive_plane(a, a.base_hhl, k, cell);
}

// rho = P / (R_D * T * (1.0 + (R_V / R_D - 1.0) * QV - load)), load summed from 0.0 in the caller's order (model_io.derive)
__device__ __forceinline__ double derive_rho(const DeriveArgs &a, int k, long cell)
{
    const double P = (double)derive_plane(a, a.base_p, k, cell), T = (double)derive_plane(a, a.base_t, k, cell),
                 QV = (double)derive_plane(a, a.base_qv, k, cell);
    double load = 0.0;
    for (int j = 0; j < a.n_load; ++j) load = load + (double)derive_plane(a, a.base_load[j], k, cell);
    return P / (a.r_d * T * (1.0 + a.rv_rd_m1 * QV - load));
}

__device__ __forceinline__ float derive_value(const DeriveArgs &a, int v, int k, long cell, double rho)
{
    switch (a.recipe[v]) {
    case CPOL_RECIPE_COPY: return derive_plane(a, a.base_src[v], k, cell);
    case CPOL_RECIPE_HALF_MEAN: return derive_half_mean(a, a.base_src[v], k, cell);
    case CPOL_RECIPE_RHO: return (float)rho;
    case CPOL_RECIPE_TIMES_RHO: return (float)((double)derive_plane(a, a.base_src[v], k, cell) * rho);    // the unrounded rho
    default: return 0.0f;
    }
}

// Raw planes -> V, H, HT.  A workgroup takes 64 cells x kc levels: lanes run along x when they read the planes, the
// values go through LDS ([cell][level][variable], rows of `rowlen` words), and each wavefront then stores consecutive
// words of one cell's run of kc * n_vars floats (VEC4: 16 bytes per lane; the host picks it when every run starts on a
// 16-byte boundary) -- instead of k_stage_variable's 4-byte stores n_vars * 4 bytes apart.
// grid (cells / 64, levels / kc), 256 threads, (64 * rowlen + 64 * (kc + 1)) * 4 bytes of dynamic LDS.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_model_derive(const DeriveArgs a)
{
    extern __shared__ __align__(16) float derive_lds[];
    float *hrow = derive_lds + 64 * a.rowlen;
    const int c = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long cell0 = (long)blockIdx.x * 64, cell = cell0 + c;
    const int k0 = blockIdx.y * a.kc, kn = min(a.kc, a.nz - k0);
    if (cell < a.ncell) {
        for (int l = w; l < kn; l += 4) {
            const int k = k0 + l;
            const double rho = derive_rho(a, k, cell);
            float *row = derive_lds + c * a.rowlen + l * a.n_vars;
            for (int v = 0; v < a.n_vars; ++v) row[v] = derive_value(a, v, k, cell, rho);
            hrow[c * (a.kc + 1) + l] = derive_height(a, k, cell);
        }
        if (blockIdx.y == 0 && w == 0) a.HT[cell] = make_float2(derive_height(a, 0, cell), derive_height(a, a.nz - 1, cell));
    }
    __syncthreads();
    const int run = kn * a.n_vars;
    const int n_here = (int)min(64L, a.ncell - cell0);
    for (int cc = w; cc < n_here; cc += 4) {
        float *dst = a.V + ((cell0 + cc) * a.nz + k0) * a.n_vars;
        const float *src = derive_lds + cc * a.rowlen;
        if (VEC4) {
            for (int i = c * 4; i < run; i += 256) *(float4 *)(dst + i) = *(const float4 *)(src + i);
        } else {
            for (int i = c; i < run; i += 64) dst[i] = src[i];
        }
    }
    for (int i = threadIdx.x; i < n_here * kn; i += 256) {
        const int cc = i / kn, l = i - cc * kn;
        a.H[(cell0 + cc) * a.nz + k0 + l] = hrow[cc * (a.kc + 1) + l];
    }
}
