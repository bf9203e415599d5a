// Host check of cpol_gate_ops.h (tests/test_gate_ops_cpu.py): the finish record of k_gate1_ray equals its sources field by
// field for two sweeps that differ in every field, its size is a whole number of 64-byte lines, and `generic` is set for
// each of its five triggers and for none of the rest.
#include <cstdio>

#include "cpol_gate_ops.h"

// stand-ins with the field names of FinalArgs (cpol_final.inl) and GateArgs (cpol_gate.inl) that the filler reads
struct Final {
    float *ZH, *ZV, *ZDR, *KDP, *DELTA_HV, *RHOHV, *ATT_H, *ATT_V;
    double *RVEL, *mask;
    signed char *mask8;
    const signed char *sub_mask;
    const float *vals, *elev;
    const double *geo, *nyquist, *wgate, *proj;
    float *sz_total;
    double *model_vars;
    int n_h, var_u, var_v, var_w, n_rays, n_gates, n_sub, with_attenuation;
    float c_zh, c_kdp, c_2w, res_km;
};
struct Gate { float *sk, *sh, *sv; };

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static float f32[64];
static double f64[512];
static signed char i8[64];

static Final make_final(int k)
{
    Final f{};
    f.ZH = f32 + 1 + k; f.ZV = f32 + 3 + k; f.ZDR = f32 + 5 + k; f.KDP = f32 + 7 + k; f.DELTA_HV = f32 + 9 + k;
    f.RHOHV = f32 + 11 + k; f.ATT_H = f32 + 13 + k; f.ATT_V = f32 + 15 + k;
    f.RVEL = f64 + 1 + k; f.mask = f64 + 3 + k; f.mask8 = i8 + 1 + k;
    f.sub_mask = i8 + 3 + k; f.vals = f32 + 17 + k; f.elev = f32 + 19 + k;
    f.geo = f64 + 5 + k; f.nyquist = f64 + 7 + k;
    f.n_h = 3 + k; f.var_u = 4 + k; f.var_v = 6 + k; f.var_w = 8 + k; f.n_rays = 360 + k; f.n_gates = 500 + k; f.n_sub = 1;
    f.with_attenuation = k;
    f.c_zh = 1.5f + k; f.c_kdp = 2.5f + k; f.c_2w = 3.5f + k; f.res_km = 0.3f + k;
    return f;
}

static void check_fields(int k)
{
    const Final f = make_final(k);
    const Gate g{f32 + 21 + k, f32 + 23 + k, f32 + 25 + k};
    const int sub_h[2] = {2 - k, 9};
    const double sub_w[2] = {0.25 + k, 9.0};
    const Gate1FinishOps o = gate1_finish_ops(f, g, sub_h, sub_w);
    CHECK(o.ZH == f.ZH && o.ZV == f.ZV && o.ZDR == f.ZDR && o.KDP == f.KDP && o.DELTA_HV == f.DELTA_HV && o.RHOHV == f.RHOHV);
    CHECK(o.ATT_H == f.ATT_H && o.ATT_V == f.ATT_V && o.RVEL == f.RVEL && o.mask == f.mask && o.mask8 == f.mask8);
    CHECK(o.sk == g.sk && o.sh == g.sh && o.sv == g.sv);
    CHECK(o.sub_mask == f.sub_mask && o.vals == f.vals && o.elev == f.elev && o.nyquist == f.nyquist);
    CHECK(o.geo_row == f.geo + 8 * sub_h[0] && o.geo_stride == 8L * f.n_h);      // ray r, sub-beam 0: geo + (r * n_h + sub_h[0]) * 8
    CHECK(o.sub_w0 == sub_w[0]);
    CHECK(o.var_u == f.var_u && o.var_v == f.var_v && o.var_w == f.var_w && o.n_rays == f.n_rays && o.n_gates == f.n_gates);
    CHECK(o.with_attenuation == f.with_attenuation);
    CHECK(o.c_zh == f.c_zh && o.c_kdp == f.c_kdp && o.c_2w == f.c_2w && o.res_km == f.res_km);
    CHECK(o.generic == 0);
    for (int q = 0; q < (int)(sizeof o.pad_ / sizeof o.pad_[0]); ++q) CHECK(o.pad_[q] == 0);
    // without RVEL nothing reads the geometry row: the sweep leaves geo and sub_h unset
    Final nr = f;
    nr.RVEL = nullptr; nr.geo = nullptr;
    const Gate1FinishOps p = gate1_finish_ops(nr, g, (const int *)nullptr, sub_w);
    CHECK(p.RVEL == nullptr && p.geo_row == nullptr && p.generic == 0);
}

int main()
{
    CHECK(sizeof(Gate1FinishOps) % 64 == 0 && alignof(Gate1FinishOps) == 64);
    check_fields(0);
    check_fields(1);               // (every source value differs from the first sweep's: no field is checked against a constant)
    // generic: each trigger alone
    {
        const Gate g{f32, f32, f32};
        const int sub_h[1] = {0};
        const double sub_w[1] = {1.0};
        Final f = make_final(0);
        f.sz_total = f32; CHECK(gate1_finish_ops(f, g, sub_h, sub_w).generic == 1);
        f = make_final(0); f.model_vars = f64; CHECK(gate1_finish_ops(f, g, sub_h, sub_w).generic == 1);
        f = make_final(0); f.wgate = f64; CHECK(gate1_finish_ops(f, g, sub_h, sub_w).generic == 1);
        f = make_final(0); f.proj = f64; CHECK(gate1_finish_ops(f, g, sub_h, sub_w).generic == 1);
        f = make_final(0); f.n_sub = 2; CHECK(gate1_finish_ops(f, g, sub_h, sub_w).generic == 1);
        f = make_final(0); f.n_sub = 0; CHECK(gate1_finish_ops(f, g, sub_h, sub_w).generic == 1);
        // and nothing else: no RVEL, no mask arrays, no Nyquist table, no attenuation
        f = make_final(0); f.RVEL = nullptr; f.mask = nullptr; f.mask8 = nullptr; f.nyquist = nullptr; f.with_attenuation = 0;
        CHECK(gate1_finish_ops(f, g, sub_h, sub_w).generic == 0);
    }
    if (fails) return 1;
    std::printf("GATE_OPS_OK %zu bytes\n", sizeof(Gate1FinishOps));
    return 0;
}
