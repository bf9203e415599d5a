// cpol_species.inl -- hydrometeor contributions (cpol_species, include/cosmo_pol_amd.h states the rule; cosmo_pol_amd/species.py
// states it in NumPy): k_species turns the per-species rows sz_integ[gate][species][12] of a sweep into the per-species radar
// fields, the presence bits, the dominant species and its share.  Included by cosmo_pol_hip.hip; -ffp-contract=off like every
// kernel of the library: each statement below is the float32 operation the rule names.
//
// Shape: one lane per gate, the species in a loop.  A gate's rows are contiguous and 16-byte aligned (48 bytes each), so a row is
// three 16-byte loads; a wavefront's loads of one species touch 64 rows 48 * n_hydro bytes apart, and the three loads of a row and
// the loop over the species between them use every byte of the lines they touch.  The per-species stores run along the gates:
// 256 contiguous bytes per wavefront and array.  dominant / present / share are formed in registers as the loop goes.  The
// kernel is bound by its memory traffic (48 * n_hydro bytes in, 4 bytes per requested field and species out, ~30 float32
// operations per row, one float64 atan2 per row only when DELTA_HV is asked for); an array that was not asked for costs neither
// its store nor the operations that only it needs (the pointers are kernel arguments: every such branch is wave-uniform).
#ifndef CPOL_SPECIES_THREADS
#define CPOL_SPECIES_THREADS 256
#endif

// the arrays of a cpol_species in the order of the struct: the placement plan's slots and SpeciesArgs::f
enum { SP_ZH = 0, SP_ZV, SP_ZDR, SP_KDP, SP_RHOHV, SP_DHV, SP_ATTH, SP_ATTV, SP_FIELDS, SP_DOMINANT = SP_FIELDS, SP_PRESENT, SP_SHARE, SP_SZ, SP_N };

struct SpeciesArgs {
    const float *sz_integ;      // [n_rg][n_hydro][12]
    const float *zh_final;      // [n_rg]: the call's ZH as delivered
    float *f[SP_FIELDS];        // each [n_hydro][n_rg] or NULL
    unsigned char *dominant, *present;      // [n_rg] or NULL
    float *share;               // [n_rg] or NULL
    long n_rg;
    int n_hydro;
    float c_zh, c_kdp, c_2w;
};

__global__ __launch_bounds__(CPOL_SPECIES_THREADS) void k_species(SpeciesArgs a)
{
    const long rg = (long)blockIdx.x * CPOL_SPECIES_THREADS + threadIdx.x;
    if (rg >= a.n_rg) return;
    const float qnan = __builtin_nanf("");
    const float two_pi = (float)(2 * 3.14159265358979323846);
    const float zf = a.zh_final[rg];
    const bool cut = !(zf == zf);
    const float4 *row = reinterpret_cast<const float4 *>(a.sz_integ + rg * a.n_hydro * CPOL_N_SZ);
    unsigned present = 0u, dominant = 255u;
    float best = 0.0f, total = 0.0f;
    for (int j = 0; j < a.n_hydro; ++j) {
        const float4 q0 = row[3 * j], q1 = row[3 * j + 1], q2 = row[3 * j + 2];
        float t[CPOL_N_SZ] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int c = 0; c < CPOL_N_SZ; ++c) if (t[c] == 0.0f) t[c] = qnan;       // Q5
        const long o = (long)j * a.n_rg + rg;
        // the statements of gate_finish (cpol_final.inl), in its order and with its casts
        const float b = t[0] - t[1] - t[2] + t[3];
        const float cc = t[0] + t[1] + t[2] + t[3];
        const float xs_h = two_pi * b;
        const float xs_v = two_pi * cc;
        const float zh = cut ? qnan : a.c_zh * xs_h;
        if (a.f[SP_ZH]) a.f[SP_ZH][o] = zh;
        if (a.f[SP_ZV]) a.f[SP_ZV][o] = cut ? qnan : a.c_zh * xs_v;
        if (a.f[SP_ZDR]) a.f[SP_ZDR][o] = cut ? qnan : xs_h / xs_v;
        if (a.f[SP_KDP]) a.f[SP_KDP][o] = cut ? qnan : a.c_kdp * (t[10] - t[8]);
        if (a.f[SP_ATTH]) a.f[SP_ATTH][o] = 4.343e-3f * (a.c_2w * t[11]);
        if (a.f[SP_ATTV]) a.f[SP_ATTV][o] = 4.343e-3f * (a.c_2w * t[9]);
        if (a.f[SP_RHOHV]) {
            const float t47 = t[4] + t[7], t65 = t[6] - t[5];
            const float aa = t47 * t47 + t65 * t65;
            a.f[SP_RHOHV][o] = cut ? qnan : sqrtf(aa / (b * cc));
        }
        if (a.f[SP_DHV]) a.f[SP_DHV][o] = (float)atan2((double)(t[5] - t[6]), (double)(-t[4] - t[7]));
        // present, dominant (a strict comparison: a tie keeps the lower slot) and the sum of the share, species ascending
        if (zh == zh) {
            present |= 1u << j;
            if (dominant == 255u || zh > best) { dominant = (unsigned)j; best = zh; }
            total = total + zh;
        }
    }
    if (a.present) a.present[rg] = (unsigned char)present;
    if (a.dominant) a.dominant[rg] = (unsigned char)dominant;
    if (a.share) a.share[rg] = dominant == 255u ? qnan : best / total;
}
