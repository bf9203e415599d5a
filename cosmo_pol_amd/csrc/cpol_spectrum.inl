// cpol_spectrum.inl -- Doppler scheme 3: the Doppler spectrum of every gate.
//
// Reference functions replaced (wolfidan/cosmo_pol):
//   get_doppler_spectrum            scatter/doppler_scatter.py:603-716
//   get_diameter_from_rad_vel       scatter/doppler_scatter.py:545-600
//   get_refl                        scatter/doppler_c.c:11-32
//   per-sub-beam attenuation, weights, accumulation   scatter/doppler_scatter.py:297-305, 353-391
//   RVEL from the spectrum, aliasing                  scatter/doppler_scatter.py:422-437
//   spectral_width_turb / _motion, broaden_spectrum   scatter/doppler_scatter.py:360-369, 727-801
// Hydrometeors with power-law fall speeds (R, S, G, H, I) and, since round 6, the melting species (mS, mG): their fall
// speed V(D) = phi V_rain(D_r(D)) + (1 - phi) V_dry(D) has no closed inverse, the reference inverts it at EVERY gate by
// linear interpolation over the n_d nodes (V(D_k), D_k), D_k = linspace(d_min(fw), d_max(fw), n_d) -- `set_psd` clears the
// interpolator, hydrometeors.py:1426,1474; get_D_from_V :480-500 -- and evaluates N(D) on the FLOAT32 copy of that grid with
// NumPy's promotion rules (float32 powers of the float32 diameters, float64 wherever the float64 wet fraction enters:
// melt_psd32 below follows the statements of hydrometeors.py:372-439 operand by operand).
// float32 / float64 follow NumPy-2 promotion of the reference
// statements (see oracle/cosmo_pol_oracle/spectrum.py); float32 libm values are float64
// results rounded once.  Quirks kept: the diameter clamp of hydrometeor j also re-clamps
// the columns before it (:583-586); the radar constant carries K^2 squared (:709); the
// attenuation of the r-th VALID gate of a hydrometeor is added to gate r (:305).
// Departure: table indices outside [0, n_d] (possible through that clamp quirk; the C
// reference then reads out of bounds) are clamped.

#define CPOL_SPEC_THREADS 256
#define CPOL_SPEC_MAX_H CPOL_MAX_HYDRO

struct SpecArgs {
    const float *vals;          // [n_vars][n_sbg]
    const signed char *mask;    // [n_sbg]
    const float *elev;          // folded elevation [n_sbg]
    const int *key;             // [n_hydro][n_sbg]
    const double *par;          // [n_hydro][CPOL_MAX_PAR][n_sbg]
    const double *wgate;        // [n_sbg] or NULL
    const double *geo;          // [n_rays][n_h][8]
    const int *sub_h;
    const double *varray;       // [n_v]
    float *beam;                // [n_sbg][n_v] float32 spectrum of every sub-beam gate
    long n_sbg;
    int n_gates, n_sub, n_h, n_v;
    int var_u, var_v, var_w, var_rho, var_t;
    float c_spec;               // (float)(wavelength^4 / (pi^5 K^2 K^2))
    int n_melt_rows;            // 0, or 2 when a melting species is staged: rows of n_d float64 fall speeds in front of the float32 part of the LDS image
};

__device__ __forceinline__ float clamp_pair(float D, float d_min, float d_max)
{
    if (D >= d_max) D = d_max;
    if (D <= d_min) D = d_min;
    return D;
}

// a float32 matrix compared with the float64 limits of a melting species (shape (1,) arrays: the comparison promotes to float64,
// the assignment rounds the limit to float32; doppler_scatter.py:585-586)
__device__ __forceinline__ float clamp_pair64(float D, double d_min, double d_max)
{
    if ((double)D >= d_max) D = (float)d_max;
    if ((double)D <= d_min) D = (float)d_min;
    return D;
}

// NumPy's float32 power of a float32 array by a Python float (weak scalar -> float32): powf, taken as the float64 result
// rounded once; x**2 is NumPy's square fast path
__device__ __forceinline__ float powf32(float x, double y)
{
    if (y == 2.0) return x * x;
    return (float)pow((double)x, (double)(float)y);
}

// The melting species at ONE gate (hydrometeors.py:303-478).  fw, lam_r, q: float64 as the classification left them.
struct MeltGate {
    double fw, fw2, phi, lam_r, q;
    double d_min, d_max, step;       // the gate's diameter range and (d_max - d_min) / (n_d - 1)
};

// float64 diameter D: mass, D_r, fall speed; `Nraw` = rain N(D_r) V_rain(D_r) / V(D) dD_r/dD (get_N without prop_factor)
__device__ __forceinline__ void melt_terms64(const cpol_hydro_desc &d, const MeltGate &g, double D, double &M, double &V, double &Nraw)
{
    const double pi6 = 3.14159265358979323846 / 6;
    auto mass = [&](double x) { return g.fw2 * (d.r_a * pow(x, d.r_b)) + (1.0 - g.fw2) * (d.a * (d.b == 2.0 ? x * x : pow(x, d.b))); };
    auto d_r = [&](double x) { return pow((mass(x) / (pi6 * pow(x, 3.0))) / 1.0e-6, 1 / 3.) * x; };     // RHO_W = 1e-6 kg mm-3
    M = mass(D);
    const double Dr = d_r(D);
    const double dDr = (d_r(D + 0.01) - Dr) / 0.01;
    const double sq = sqrt(Dr);                                             // rain: mu = beta = 0.5, nu = 1
    const double Nr = (d.r_n0 * sq) * exp(-(g.lam_r * Dr));
    const double Vr = d.r_alpha * sq;
    const double Vd = d.alpha * pow(D, d.beta);
    V = g.phi * Vr + (1 - g.phi) * Vd;
    Nraw = Nr * Vr / V * dDr;
}

// float32 diameter D32 (a node of the float32 copy of the gate's grid): get_N as NumPy evaluates it on a float32 array --
// a D^b, pi/6 D^3, alpha_dry D^beta_dry and D + 0.01 in float32; everything the float64 wet fraction touches in float64
__device__ __forceinline__ double melt_psd32(const cpol_hydro_desc &d, const MeltGate &g, float D32, double prop)
{
    const float pi6_32 = (float)(3.14159265358979323846 / 6);
    auto d_r = [&](float x) {
        const float m_rain = (float)d.r_a * powf32(x, d.r_b), m_dry = (float)d.a * powf32(x, d.b);
        const double M = g.fw2 * (double)m_rain + (1.0 - g.fw2) * (double)m_dry;
        const float vol = pi6_32 * powf32(x, 3.0);
        return pow((M / (double)vol) / 1.0e-6, 1 / 3.) * (double)x;
    };
    const double Dr = d_r(D32);
    const double dDr = (d_r(D32 + 0.01f) - Dr) / 0.01;
    const double sq = sqrt(Dr);
    const double Nr = (d.r_n0 * sq) * exp(-(g.lam_r * Dr));
    const double Vr = d.r_alpha * sq;
    const float Vd = (float)d.alpha * powf32(D32, d.beta);
    const double V = g.phi * Vr + (1 - g.phi) * (double)Vd;
    return (prop * Nr) * Vr / V * dDr;
}

// one workgroup per sub-beam gate
__global__ __launch_bounds__(CPOL_SPEC_THREADS) void k_spec_gate(HydroSet hs, SpecSet ss, SpecArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds_spec[];
    const long sbg = blockIdx.x;
    const int tid = threadIdx.x;
    const long n = a.n_sbg;
    float *out = a.beam + sbg * a.n_v;
    for (int v = tid; v < a.n_v; v += CPOL_SPEC_THREADS) out[v] = 0.0f;
    if (a.mask[sbg] != 0) return;
    if (a.wgate && a.wgate[sbg] == 0.0) return;

    // hydrometeors present at this gate, in slot order
    int present[CPOL_SPEC_MAX_H], n_p = 0;
    for (int j = 0; j < hs.n_hydro; ++j)
        if (a.key[(long)j * n + sbg] >= 0) present[n_p++] = j;
    if (n_p == 0) return;
    const int n_d = hs.h[present[0]].d.n_d;
    // LDS: [2][n_d] float64 fall speeds of the (at most two) melting species + [CPOL_SPEC_THREADS] float64 scratch, then
    // [n_hydro][n_d] float32 N x rcs, [n_hydro][n_v] float32 edge diameters
    double *VL = reinterpret_cast<double *>(lds_spec);                        // [n_melt_rows][n_d]
    double *redL = VL + (long)a.n_melt_rows * n_d;                            // [CPOL_SPEC_THREADS] (with melting species only)
    float *prodL = reinterpret_cast<float *>(redL + (a.n_melt_rows ? CPOL_SPEC_THREADS : 0));       // [n_p][n_d]
    float *DL = prodL + (long)hs.n_hydro * n_d;                               // [n_p][n_v]
    MeltGate mg[2];
    int melt_of[CPOL_SPEC_MAX_H];                       // present species -> 0 / 1 (its row of VL), or -1
    float dmin32[CPOL_SPEC_MAX_H], step32[CPOL_SPEC_MAX_H];
    int n_melt = 0;

    // ---- N(D) x rcs per diameter bin (float32 product of float32 operands) ----
    for (int p = 0; p < n_p; ++p) {
        const int j = present[p];
        const HydroDev &h = hs.h[j];
        const cpol_hydro_desc &d = h.d;
        const int key = a.key[(long)j * n + sbg];
        const SpecDev &sd = ss.s[j];
        const float *rcs = sd.rcs32 + (long)(key - h.key_base) * d.n_d;
        const double *P = a.par + ((long)j * CPOL_MAX_PAR) * n + sbg;
        melt_of[p] = -1;
        if (d.psd_family == CPOL_PSD_MELTING && n_melt < a.n_melt_rows) {
            // ---- a melting species: its grid, fall speeds and PSD belong to THIS gate's wet fraction ----
            MeltGate &g = mg[n_melt];
            g.q = P[0]; g.fw = P[n]; g.lam_r = P[2 * n];
            g.fw2 = g.fw * g.fw;                                            // fw ** 2: NumPy's square
            g.phi = 0.246 * g.fw + (1 - 0.246) * pow(g.fw, 7.0);
            g.d_max = g.fw * d.r_dmax + (1 - g.fw) * d.s_dmax;              // hydrometeors.py:336-339
            g.d_min = g.fw * d.r_dmin + (1 - g.fw) * d.s_dmin;
            g.step = (g.d_max - g.d_min) / (double)(d.n_d - 1);
            double *Vrow = VL + (long)n_melt * n_d;
            // integrate_M on the float64 grid (vlinspace, utilities.py:158-173; :462-478) and, on the same nodes, the fall
            // speeds of get_D_from_V (np.linspace: the same nodes but for the last, which is d_max itself)
            double msum = 0.0;
            for (int k = tid; k < d.n_d; k += CPOL_SPEC_THREADS) {
                const double D = g.d_min + g.step * (double)k;
                double M, V, Nraw;
                melt_terms64(d, g, D, M, V, Nraw);
                msum += Nraw * M;
                if (k == d.n_d - 1 && D != g.d_max) { double M1, N1; melt_terms64(d, g, g.d_max, M1, V, N1); }
                Vrow[k] = V;
            }
            redL[tid] = msum;
            __syncthreads();
            for (int off = CPOL_SPEC_THREADS / 2; off >= 1; off >>= 1) {
                if (tid < off) redL[tid] += redL[tid + off];
                __syncthreads();
            }
            const double dD = (g.d_min + g.step * 1.0) - (g.d_min + g.step * 0.0);
            const double prop = g.q / (redL[0] * dD);                       // q / integrate_M (:1428, :1475)
            __syncthreads();                                                // (redL is reused by the second melting species)
            // the float32 grid of the spectrum: D[:, j] = np.linspace(d_min, d_max, n_d) stored as float32
            const float D0 = (float)g.d_min, D1 = (float)(1.0 * g.step + g.d_min);
            dmin32[p] = D0; step32[p] = D1 - D0;
            for (int k = tid; k < d.n_d; k += CPOL_SPEC_THREADS) {
                const float D32 = (k == d.n_d - 1) ? (float)g.d_max : (float)((double)k * g.step + g.d_min);
                prodL[(long)p * n_d + k] = (float)melt_psd32(d, g, D32, prop) * rcs[k];
            }
            melt_of[p] = n_melt++;
            continue;
        }
        dmin32[p] = sd.dgrid[0]; step32[p] = sd.step32;
        const double lam = P[0];
        const bool fixed_n0 = d.rule == CPOL_RULE_RAIN_1MOM || d.rule == CPOL_RULE_GRAUPEL_1MOM;
        const double N0 = (d.psd_family == CPOL_PSD_ICE_FIELD) ? P[3 * n] : (fixed_n0 ? d.n0_fixed : P[n]);
        for (int k = tid; k < d.n_d; k += CPOL_SPEC_THREADS) {
            double nk;
            if (d.psd_family == CPOL_PSD_ICE_FIELD) {
                const double x = lam * (double)sd.dgrid[k] / 1000.0;
                nk = N0 * phi23(x);
            } else {
                nk = (N0 * (double)sd.dgrid[d.n_d + k]) * exp(-(lam * (double)sd.dgrid[2 * d.n_d + k]));
            }
            prodL[(long)p * n_d + k] = (float)nk * rcs[k];
        }
    }

    // ---- diameters of the velocity-bin edges ----
    const int rs = (int)(sbg / a.n_gates);              // ray * n_sub + sub
    const int ray = rs / a.n_sub, sub = rs % a.n_sub;
    const double *gc = a.geo + ((long)ray * a.n_h + a.sub_h[sub]) * 8;
    const float th = a.elev[sbg] * 0.017453292f;        // np.deg2rad of a float32
    const float tan32 = (float)tan((double)th), sin32 = (float)sin((double)th);
    const float rho = a.vals[(long)a.var_rho * n + sbg];
    const float rho0 = a.vals[(long)a.var_rho * n + (long)rs * a.n_gates];
    const float inv_rho = 1.0f / sqrtf(rho / rho0);
    const double U = (double)a.vals[(long)a.var_u * n + sbg], V = (double)a.vals[(long)a.var_v * n + sbg],
                 W = (double)a.vals[(long)a.var_w * n + sbg];
    const double horiz = (U * gc[0] + V * gc[1]) / (double)tan32;
    float *okL = DL + (long)hs.n_hydro * a.n_v;         // [n_v] 1: wh >= 0 at this velocity (a row of the reference's D matrix)
    __syncthreads();                                    // (VL complete)
    for (int v = tid; v < a.n_v; v += CPOL_SPEC_THREADS) {
        const double wh = (double)inv_rho * (W + horiz - a.varray[v] / (double)sin32);
        const bool ok = wh >= 0.0;
        okL[v] = ok ? 1.0f : 0.0f;
        for (int p = 0; p < n_p; ++p) {
            const cpol_hydro_desc &d = hs.h[present[p]].d;
            float D = __builtin_nanf("");
            if (ok && melt_of[p] < 0) {
                D = (float)pow(wh / d.alpha, 1.0 / d.beta);
            } else if (ok) {
                // scipy.interpolate.interp1d(V_all, D_all, bounds_error=False, fill_value=nan) at wh (hydrometeors.py:494-500): for 1-D
                // float64 data SciPy hands the evaluation to np.interp -- j with V_j <= wh < V_{j+1} by binary search, D_j when wh == V_j
                // or j is the last node, else slope * (wh - V_j) + D_j -- and fills NaN outside [V_0, V_{n-1}]
                const MeltGate &g = mg[melt_of[p]];
                const double *Vrow = VL + (long)melt_of[p] * n_d;
                if (!(wh < Vrow[0]) && !(wh > Vrow[d.n_d - 1])) {
                    int lo_i = 0, hi_i = d.n_d;                            // first index with V > wh
                    while (lo_i < hi_i) {
                        const int mid = (lo_i + hi_i) >> 1;
                        if (Vrow[mid] <= wh) lo_i = mid + 1; else hi_i = mid;
                    }
                    const int j = max(0, lo_i - 1);
                    const double y_j = (j == d.n_d - 1) ? g.d_max : (double)j * g.step + g.d_min;
                    if (j == d.n_d - 1 || Vrow[j] == wh) {
                        D = (float)y_j;
                    } else {
                        const double y_n = (j + 1 == d.n_d - 1) ? g.d_max : (double)(j + 1) * g.step + g.d_min;
                        const double slope = (y_n - y_j) / (Vrow[j + 1] - Vrow[j]);
                        D = (float)(slope * (wh - Vrow[j]) + y_j);
                    }
                }
            }
            if (ok)
                for (int q = p; q < n_p; ++q) {           // clamps of this and the later species (a NaN stays a NaN)
                    if (melt_of[q] >= 0) {
                        D = clamp_pair64(D, mg[melt_of[q]].d_min, mg[melt_of[q]].d_max);
                    } else {
                        const SpecDev &sq = ss.s[present[q]];
                        D = clamp_pair(D, sq.dgrid[0], sq.dgrid[hs.h[present[q]].d.n_d - 1]);
                    }
                }
            DL[(long)p * a.n_v + v] = D;
        }
    }
    __syncthreads();

    // ---- rows = consecutive valid edges; sum N x rcs over [Da, Db) per species ----
    for (int v = tid; v + 1 < a.n_v; v += CPOL_SPEC_THREADS) {
        if (okL[v] == 0.0f || okL[v + 1] == 0.0f) continue;   // wh < 0 at one of the edges: not a row of the D matrix
        bool keep = false;
        float refl = 0.0f;
        for (int p = 0; p < n_p; ++p) {
            const float x0 = DL[(long)p * a.n_v + v], x1 = DL[(long)p * a.n_v + v + 1];
            // np.minimum / np.maximum propagate a NaN (a melting species outside its interpolator) to BOTH edges; (Db - Da) == 0
            // is then false -- the row is kept -- and the two (int) conversions of doppler_c.c give the same index: an empty bin
            const bool nan_edge = !(x0 == x0) || !(x1 == x1);
            const float Da = fminf(x0, x1), Db = fmaxf(x0, x1);
            if (nan_edge || Db - Da != 0.0f) keep = true;
            if (nan_edge) continue;
            int ia = (int)((Da - dmin32[p]) / step32[p]);
            int ib = (int)((Db - dmin32[p]) / step32[p]);
            ia = max(0, min(ia, n_d));
            ib = max(0, min(ib, n_d));
            float sum = 0.0f;
            for (int k = ia; k < ib; ++k) sum += prodL[(long)p * n_d + k];
            refl += sum * step32[p];
        }
        if (keep) out[v] = refl * a.c_spec;
    }
}

// ---- broadening of the spectrum by turbulence and antenna motion (doppler_scatter.py:360-369, 727-801) ----
// Per sub-beam, between get_doppler_spectrum and the attenuation correction: a width per gate (two standard deviations in
// m/s, added LINEARLY, :361-366), the sub-beam's switch `np.sum(width) > 0` (:368 -- one non-finite width, an EDR that is
// NaN or negative at a masked gate, makes the sum NaN and leaves the WHOLE sub-beam unbroadened), then per gate
// scipy.ndimage.gaussian_filter of the float32 row with sigma = width / v_res bins (truncate 4, mode 'reflect', float64
// accumulation in SciPy's order) and the rescale row / sum(filtered) * sum(original) in float32: a row without power
// becomes 0 / 0 = NaN and, through the sum over the sub-beams, so do the gate's spectrum and RVEL.
// Departures, for inputs the reference raises on or cannot finish: a sigma <= 1e-15 bins inside a broadened sub-beam filters as
// the identity (what gaussian_filter's own guard does; the rescale still runs); an infinite width switches the sub-beam off
// like a NaN; the radius int(4 sigma + 0.5) is cut at CPOL_BROAD_MAX_RADIUS taps (sigma > 16384 bins).
struct SpecWidthArgs {
    const float *vals;          // [n_vars][n_sbg]
    const float *elev;          // folded elevation [n_sbg] (the reference folds elev_profile in place before it gets here, Q8)
    double *sigma;              // [n_sbg] width / v_res: the filter's sigma in bins
    int *on;                    // [n_rays * n_sub] the sub-beam's switch
    long n_sbg;
    int n_gates;
    int turb, motion, var_edr;
    double range0, range_step;  // RANGE_RADAR[g] = range0 + g * range_step
    double sigma_r, sigma_theta;
    double c_near, c_far;       // A^1.5 and (1.35 A)^1.5, evaluated by the host's libm as Python does
    double motion_num, motion_den;      // (WAVELENGTH / 100) * antenna_speed and 2 pi deg2rad(3dB_beamwidth)
    double v_res;
};

// one wavefront per (ray, sub-beam).  NumPy-2 promotion of spectral_width_turb / spectral_width_motion: the float32 EDR
// times the two Python floats of the far branch stays float32, as does the float32 cosine times the motion numerator.
__global__ __launch_bounds__(64) void k_spec_width(SpecWidthArgs a)
{
    const long rs = blockIdx.x;
    const int lane = threadIdx.x;
    double sum = 0.0;
    bool finite = true;
    for (int g0 = 0; g0 < a.n_gates; g0 += 64) {
        const int g = g0 + lane;
        if (g >= a.n_gates) continue;
        const long sbg = rs * a.n_gates + g;
        double w = 0.0;
        if (a.turb) {
            const double r = a.range0 + a.range_step * (double)g;
            const float E = a.vals[(long)a.var_edr * a.n_sbg + sbg];
            double t;
            if (a.sigma_r < (0.1 * r) * a.sigma_theta) {              // sigma_r << r sigma_theta (Doviak & Zrnic p. 409)
                t = pow(((((r * (double)E) * a.sigma_theta) * a.c_near) / 0.72), 1 / 3.);
            } else {
                const float num = (E * (float)a.sigma_r) * (float)a.c_far;
                const double x = (r * a.sigma_theta) / a.sigma_r;
                const double den = pow(11. / 15. + 4. / 15. * (x * x), -3 / 2.);
                t = pow((double)num / den, 1 / 3.);
            }
            w += t;
        }
        if (a.motion) {
            const float th = a.elev[sbg] * 0.017453292f;              // np.deg2rad of a float32
            const float c32 = (float)cos((double)th);
            const float num = (float)a.motion_num * c32;
            w += (double)num / a.motion_den;
        }
        a.sigma[sbg] = w / a.v_res;
        if (!(fabs(w) <= 1.7976931348623157e308)) finite = false;     // NaN or infinite
        else sum += w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += shfl_f64(sum, lane ^ off);
    const bool all_finite = __all(finite ? 1 : 0) != 0;
    if (lane == 0) a.on[rs] = (all_finite && sum > 0.0) ? 1 : 0;
}

#define CPOL_TURB_A 1.6                 // global_constants.py:124
#define CPOL_BROAD_CHUNK 256            // filter taps staged in LDS at a time
#define CPOL_BROAD_MAX_OUT 17           // bins per thread: 4097 bins / 256 threads, 1024 bins / 64 threads
#ifndef CPOL_BROAD_WAVE_BINS
#define CPOL_BROAD_WAVE_BINS 1024       // rows up to this length are filtered by one wavefront, longer ones by 256 threads
#endif
#define CPOL_BROAD_MAX_RADIUS 65536

template <int T> __device__ __forceinline__ float broad_sum32(float x, float *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    if (T > 64) {
        __syncthreads();                                  // (red may still be read from the previous sum)
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
        __syncthreads();
        x = red[0];
        for (int w = 1; w < T / 64; ++w) x += red[w];
    }
    return x;
}

template <int T> __device__ __forceinline__ double broad_sum64(double x, double *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += shfl_f64(x, (threadIdx.x & 63) ^ off);
    if (T > 64) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
        __syncthreads();
        x = red[0];
        for (int w = 1; w < T / 64; ++w) x += red[w];
    }
    return x;
}

// One row of broaden_spectrum by the T threads of a workgroup: `in` -> `out` (may be the same row), sigma in bins.
// xL: [n_v] floats of LDS.  The taps follow NI_Correlate1D's symmetric form: the centre tap, then the pairs
// (x[i - k] + x[i + k]) w[k] from k = radius down to 1, accumulated in float64 and rounded once; the weights
// exp(-0.5 / sigma^2 * k^2) / sum are made CPOL_BROAD_CHUNK at a time, so LDS does not grow with sigma.  Reflection
// (d c b a | a b c d | d c b a) by position modulo 2 n_v: any radius works.
template <int T> __device__ void broaden_row(const float *in, float *out, int n_v, double sigma, float *xL)
{
    __shared__ double wL[CPOL_BROAD_CHUNK];
    __shared__ double red64[4];
    __shared__ float red32[4];
    const int tid = threadIdx.x;
    float part = 0.0f;
    for (int v = tid; v < n_v; v += T) { const float x = in[v]; xL[v] = x; part += x; }
    __syncthreads();
    const float orig = broad_sum32<T>(part, red32);
    double acc[CPOL_BROAD_MAX_OUT];
#pragma unroll
    for (int o = 0; o < CPOL_BROAD_MAX_OUT; ++o) { const int v = tid + o * T; acc[o] = v < n_v ? (double)xL[v] : 0.0; }
    if (sigma > 1e-15) {                                  // (gaussian_filter skips an axis whose sigma is not above 1e-15)
        const double r4 = 4.0 * sigma + 0.5;
        const int radius = r4 < (double)CPOL_BROAD_MAX_RADIUS ? (int)r4 : CPOL_BROAD_MAX_RADIUS;
        const double c = -0.5 / (sigma * sigma);
        double ws = 0.0;
        for (int k = 1 + tid; k <= radius; k += T) ws += exp(c * ((double)k * (double)k));
        const double total = 1.0 + 2.0 * broad_sum64<T>(ws, red64);
        const double w0 = 1.0 / total;
#pragma unroll
        for (int o = 0; o < CPOL_BROAD_MAX_OUT; ++o) acc[o] = acc[o] * w0;
        const int period = 2 * n_v;
        for (int k_hi = radius; k_hi >= 1; k_hi -= CPOL_BROAD_CHUNK) {
            const int cnt = min(CPOL_BROAD_CHUNK, k_hi);
            __syncthreads();                              // (the previous chunk has been read)
            for (int t = tid; t < cnt; t += T) { const double k = (double)(k_hi - t); wL[t] = exp(c * (k * k)) / total; }
            __syncthreads();
            // (bins outside, taps inside.  Taps outside with the bins of a thread as independent chains needs the two reflected
            // positions of every bin in registers: 143 VGPRs, 240 us instead of 186 us on the 360 x 60 x 257 sweep of DESIGN.md 3.10)
#pragma unroll
            for (int o = 0; o < CPOL_BROAD_MAX_OUT; ++o) {
                const int v = tid + o * T;
                if (v >= n_v) continue;
                int mL = (v - k_hi) % period; if (mL < 0) mL += period;
                int mR = (v + k_hi) % period;
                double s = acc[o];
                for (int t = 0; t < cnt; ++t) {
                    const float xl = xL[mL < n_v ? mL : period - 1 - mL], xr = xL[mR < n_v ? mR : period - 1 - mR];
                    s += ((double)xl + (double)xr) * wL[t];
                    mL = mL + 1 == period ? 0 : mL + 1;
                    mR = mR == 0 ? period - 1 : mR - 1;
                }
                acc[o] = s;
            }
        }
    }
    float y[CPOL_BROAD_MAX_OUT];
    part = 0.0f;
#pragma unroll
    for (int o = 0; o < CPOL_BROAD_MAX_OUT; ++o) { y[o] = (float)acc[o]; if (tid + o * T < n_v) part += y[o]; }
    const float conv = broad_sum32<T>(part, red32);
#pragma unroll
    for (int o = 0; o < CPOL_BROAD_MAX_OUT; ++o) { const int v = tid + o * T; if (v < n_v) out[v] = y[o] / conv * orig; }
}

struct SpecBroadenArgs {
    const float *in;            // [n_rows][n_v]
    float *out;                 // [n_rows][n_v] (the sweep filters its sub-beam spectra in place)
    const double *sigma;        // [n_rows] in bins
    const int *on;              // [n_rows / rows_per_switch] or NULL (every row)
    int rows_per_switch;        // n_gates
    int n_v;
};

// one workgroup per row (= sub-beam gate): 64 threads for rows up to CPOL_BROAD_WAVE_BINS bins, 256 beyond
template <int T> __global__ __launch_bounds__(T) void k_spec_broaden(SpecBroadenArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds_row[];
    const long row = blockIdx.x;
    if (a.on && !a.on[row / a.rows_per_switch]) return;   // rows of a sub-beam whose switch is off are not touched
    broaden_row<T>(a.in + row * a.n_v, a.out + row * a.n_v, a.n_v, a.sigma[row], lds_row);
}

// ---- per (ray, sub-beam): attenuation of the spectrum (doppler_scatter.py:297-305, 372-384)
struct SpecAttenArgs {
    const int *key;             // [n_hydro][n_sbg]
    const double *res;          // [n_hydro][n_sbg][12]
    float *beam;                // [n_sbg][n_v]
    long n_sbg;
    int n_gates, n_v, n_hydro;
    double c_att;               // 4.343e-3 * 2 * wavelength
    double res_km;              // radial_res / 1000.
};

__global__ __launch_bounds__(64) void k_spec_atten(SpecAttenArgs a)
{
    extern __shared__ double lds_att[];                 // [n_gates]
    const long rs = blockIdx.x;
    const int lane = threadIdx.x;
    const long base = rs * a.n_gates;
    for (int g = lane; g < a.n_gates; g += 64) lds_att[g] = 0.0;
    __syncthreads();
    for (int j = 0; j < a.n_hydro; ++j) {
        int count = 0;
        for (int g0 = 0; g0 < a.n_gates; g0 += 64) {
            const int g = g0 + lane;
            const bool valid = g < a.n_gates && a.key[(long)j * a.n_sbg + base + g] >= 0;
            const unsigned long long m = __ballot(valid);
            if (valid) {
                const int rank = count + __popcll(m & ((1ull << lane) - 1ull));
                double ah = a.c_att * a.res[((long)j * a.n_sbg + base + g) * CPOL_N_SZ + 11];
                ah *= a.res_km;
                if (ah == ah) lds_att[rank] += ah;        // nansum_arr: NaN counts as 0
            }
            count += __popcll(m);
        }
        __syncthreads();
    }
    if (lane == 0) {
        double c = 0.0;
        for (int g = 0; g < a.n_gates; ++g) { c += lds_att[g]; lds_att[g] = c; }
    }
    __syncthreads();
    for (int g = 0; g < a.n_gates; ++g) {
        float *row = a.beam + (base + g) * a.n_v;
        float s = 0.0f;
        for (int v = lane; v < a.n_v; v += 64) { const float x = row[v]; if (x == x) s += x; }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if (!(s > 0.0f)) continue;                        // wave-uniform
        const float db = 10.0f * (float)log10((double)s);
        const double frac = (double)s / pow(10.0, 0.1 * ((double)db - lds_att[g]));
        for (int v = lane; v < a.n_v; v += 64) row[v] = (float)((double)row[v] / frac);
    }
}

// ---- accumulation over sub-beams, RVEL (doppler_scatter.py:386-391, 422-437)
struct SpecFinalArgs {
    const float *beam;          // [n_sbg][n_v]
    const double *sub_w;
    const double *wgate;        // per-gate weights (scheme 'ml') or NULL
    const double *varray;
    const double *nyquist;      // [n_rays] or NULL
    const double *sens_thr;     // [n_gates] dBZ threshold per gate, or NULL (no sensitivity cut)
    double *spectrum;           // [n_rg][n_v]
    double *RVEL;               // [n_rg]
    int n_rays, n_gates, n_sub, n_v;
};

__global__ __launch_bounds__(64) void k_spec_final(SpecFinalArgs a)
{
    const long rg = blockIdx.x;
    const int lane = threadIdx.x;
    const int ray = (int)(rg / a.n_gates), gate = (int)(rg % a.n_gates);
    const long sbg0 = (long)ray * a.n_sub * a.n_gates + gate;
    double num = 0.0, den = 0.0;
    for (int v = lane; v < a.n_v; v += 64) {
        double acc = 0.0;
        for (int s = 0; s < a.n_sub; ++s) {
            const long sbg = sbg0 + (long)s * a.n_gates;
            const float b = a.beam[sbg * a.n_v + v];
            // beam_spectrum *= quad_weight: float32 x python float -> float32; an array of
            // float64 weights multiplies in float64 and stores float32
            const float wb = a.wgate ? (float)((double)b * a.wgate[sbg]) : b * (float)a.sub_w[s];
            acc += (double)wb;
        }
        // cut_at_sensitivity as get_PPI / get_RHI call it (a list of lists of radials,
        // doppler_scatter.py:839-850) censors the spectrum BIN BY BIN with
        // 10 log10(spectrum) < threshold(r); the gate-level ZH mask does not touch it.  (The cut
        // runs after RVEL was derived from the uncensored spectrum, :422-437.)
        a.spectrum[rg * a.n_v + v] =
            (a.sens_thr && 10.0 * log10(acc) < a.sens_thr[gate]) ? __builtin_nan("") : acc;
        if (acc == acc) { num += a.varray[v] * acc; den += acc; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        num += shfl_f64(num, lane ^ off);
        den += shfl_f64(den, lane ^ off);
    }
    if (lane == 0) {
        double rv = num / den;
        if (a.nyquist) {
            const double nyq = a.nyquist[ray], pi = 3.14159265358979323846;
            const double theta = (rv + nyq) / (2 * nyq) * pi - pi / 2.;
            const double fold = atan(tan(theta));
            rv = (fold + pi / 2) * (2 * nyq) / pi - nyq;
        }
        a.RVEL[rg] = rv;
    }
}

// ---- spectrum moments (cpol_spectrum_moments): power, mean velocity, width, skewness, kurtosis, peak and edges per gate ----
// Reference functions replaced (wolfidan/cosmo_pol): none -- the reference forms no moment of the spectrum but RVEL.  The
// rule is the one of include/cosmo_pol_amd.h and cosmo_pol_amd/spectrum_moments.py (`moments`), ORDER-EXACT: every sum is
// 64 lane sums over the counting bins v = l, l + 64, ... in ascending order from +0.0, then the butterfly off = 32 ... 1 in
// which every lane adds its partner's value to its own (IEEE addition commutes: the 64 lanes end with the same bits).  Only
// IEEE adds, multiplies, divides and one square root; the TU is compiled with -ffp-contract=off -fno-fast-math.
#define CPOL_SM_FIELDS 8            // POWER, VMEAN, WIDTH, SKEWNESS, KURTOSIS, VPEAK, VLOW, VHIGH (the rows of `moments`)
#define CPOL_SM_GATES_PER_BLOCK 4   // one wavefront per gate, four gates per workgroup

struct SpecMomentsArgs {
    const double *spectrum;     // [n_rg][n_v] as k_spec_final leaves it (censored bins are NaN)
    const double *varray;       // [n_v]
    double *moments;            // [8][n_rg]
    unsigned short *count;      // [n_rg] or NULL
    long n_rg;
    int n_v;
    unsigned fields;            // bit k: row k is written
    int min_bins;
    double min_power;
    int zero_rest;              // 1: the rows of `moments` nobody asked for are written as zeros (a window image)
};

__device__ __forceinline__ double spec_moments_sum(double a, int lane)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = a + shfl_f64(a, lane ^ off);
    return a;
}

// Pass 1 reads the row once (lanes on consecutive float64 bins: 512 B per wavefront load), pass 2 reads it again -- 2 KB to
// 32 KB per gate, which the cache still holds.  A gate with fewer counting bins than min_bins leaves after pass 1.
__global__ __launch_bounds__(64 * CPOL_SM_GATES_PER_BLOCK) void k_spec_moments(const SpecMomentsArgs a)
{
    const long rg = (long)blockIdx.x * CPOL_SM_GATES_PER_BLOCK + (threadIdx.x >> 6);
    if (rg >= a.n_rg) return;                                           // (wave-uniform; the kernel has no barrier)
    const int lane = threadIdx.x & 63;
    const double *__restrict__ S = a.spectrum + rg * a.n_v;
    const double *__restrict__ V = a.varray;
    double aP = 0.0, aM = 0.0, pk = -1.0;                               // (a counting bin is > min_power >= 0)
    int n = 0, ipk = 0x7fffffff, ilo = 0x7fffffff, ihi = -1;
    for (int v = lane; v < a.n_v; v += 64) {
        const double s = S[v];
        if (s == s && s > a.min_power) {
            aP = aP + s;
            aM = aM + V[v] * s;
            ++n;
            if (s > pk) { pk = s; ipk = v; }
            if (v < ilo) ilo = v;
            ihi = v;
        }
    }
    const double P = spec_moments_sum(aP, lane), M = spec_moments_sum(aM, lane);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n += __shfl(n, lane ^ off);
        ilo = min(ilo, __shfl(ilo, lane ^ off));
        ihi = max(ihi, __shfl(ihi, lane ^ off));
        const double pk2 = shfl_f64(pk, lane ^ off);
        const int ipk2 = __shfl(ipk, lane ^ off);
        if (pk2 > pk || (pk2 == pk && ipk2 < ipk)) { pk = pk2; ipk = ipk2; }     // larger value, then lower index
    }
    const double nan = __builtin_nan("");
    double out[CPOL_SM_FIELDS] = {nan, nan, nan, nan, nan, nan, nan, nan};
    if (n >= a.min_bins) {                                              // (wave-uniform; min_bins >= 1: n >= 1 here)
        const double vbar = M / P;
        double a2 = 0.0, a3 = 0.0, a4 = 0.0;
        for (int v = lane; v < a.n_v; v += 64) {
            const double s = S[v];
            if (s == s && s > a.min_power) {
                const double d = V[v] - vbar;
                const double d2 = d * d;
                a2 = a2 + d2 * s;
                a3 = a3 + (d2 * d) * s;
                a4 = a4 + (d2 * d2) * s;
            }
        }
        const double C2 = spec_moments_sum(a2, lane), C3 = spec_moments_sum(a3, lane), C4 = spec_moments_sum(a4, lane);
        const double var = C2 / P;
        const double width = sqrt(var);
        out[0] = P;
        out[1] = vbar;
        out[2] = width;
        out[3] = (C3 / P) / (var * width);
        out[4] = (C4 / P) / (var * var);
        out[5] = V[ipk];
        out[6] = V[ilo];
        out[7] = V[ihi];
    }
    if (lane != 0) return;
#pragma unroll
    for (int k = 0; k < CPOL_SM_FIELDS; ++k) {
        if ((a.fields >> k) & 1u) a.moments[(long)k * a.n_rg + rg] = out[k];
        else if (a.zero_rest) a.moments[(long)k * a.n_rg + rg] = 0.0;
    }
    if (a.count) a.count[rg] = (unsigned short)n;
}
