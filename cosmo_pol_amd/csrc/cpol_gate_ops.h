// cpol_gate_ops.h -- the operands of k_gate1_ray's finishing pass as ONE compact record, filled by the host at each launch.
// Plain C++ without HIP types, so that a host test can include it (tests/c_host/gate_ops_check.cpp, tests/test_gate_ops_cpu.py).
//
// The wavefront that takes a tile's last ticket finishes its 64 gates.  It used to take what it needs out of FinalArgs and
// GateArgs -- two of six structs that arrive by value as about 4 KB of kernel arguments -- one field at a time, each scalar
// load awaited just in front of its use (`make asm`: 20 awaited scalar rounds behind the ticket), and its vector operands in
// four to five dependent rounds: the mask code, the elevation, sub_h[s] -> the geometry row, then U, V, W.  The record holds
// exactly what a single-beam finish reads, with the geometry row base already resolved (sub_h[0] is known on the host), no
// array indexed at run time, contiguous and 64-byte aligned: it arrives in a few wide scalar loads, and every vector operand
// of the gate can be requested in one round before the species' sums are read from LDS (gate_finish_single, cpol_gate.inl).
// Nothing is kept across calls: every launch fills the record from the structs it is about to pass.
#pragma once

#include <cstddef>
#include <cstdint>

struct alignas(64) Gate1FinishOps {
    // outputs (FinalArgs, GateArgs)
    float *ZH, *ZV, *ZDR, *KDP, *DELTA_HV, *RHOHV, *ATT_H, *ATT_V;
    double *RVEL;                  // or NULL
    double *mask;                  // or NULL
    signed char *mask8;            // or NULL
    float *sk, *sh, *sv;           // the operands of the range scans
    // vector operands
    const signed char *sub_mask;
    const float *vals;
    const float *elev;
    const double *geo_row;         // FinalArgs.geo + 8 * sub_h[0]: ray r's row of 8 doubles lies at geo_row + r * geo_stride
    const double *nyquist;         // or NULL
    double sub_w0;                 // sub_w[0]
    long geo_stride;               // 8 * n_h
    int var_u, var_v, var_w;
    int n_rays, n_gates;
    int with_attenuation;
    float c_zh, c_kdp, c_2w, res_km;
    int generic;                   // a sweep gate_finish_single does not cover: the kernel calls gate_finish(FinalArgs) as before
    int pad_[11];
};
static_assert(sizeof(Gate1FinishOps) % 64 == 0 && alignof(Gate1FinishOps) == 64, "the record arrives in whole 64-byte scalar loads");
static_assert(sizeof(Gate1FinishOps) == 256, "no hidden padding: 19 pointers, 2 x 8 bytes, 11 x 4 bytes, the explicit pad");

// F: FinalArgs, G: GateArgs (templates, so that the host test can hand in plain stand-ins with the same field names);
// sub_h, sub_w: the HOST arrays of the sweep's sub-beams (the device copies are what FinalArgs points at)
template <class F, class G>
inline Gate1FinishOps gate1_finish_ops(const F &f, const G &g, const int *sub_h, const double *sub_w)
{
    Gate1FinishOps o{};
    o.generic = (f.sz_total || f.model_vars || f.wgate || f.proj || f.n_sub != 1) ? 1 : 0;
    o.ZH = f.ZH; o.ZV = f.ZV; o.ZDR = f.ZDR; o.KDP = f.KDP;
    o.DELTA_HV = f.DELTA_HV; o.RHOHV = f.RHOHV; o.ATT_H = f.ATT_H; o.ATT_V = f.ATT_V;
    o.RVEL = f.RVEL; o.mask = f.mask; o.mask8 = f.mask8;
    o.sk = g.sk; o.sh = g.sh; o.sv = g.sv;
    o.sub_mask = f.sub_mask; o.vals = f.vals; o.elev = f.elev;
    // (geo, sub_h and n_h are set for Doppler sweeps only: without RVEL nothing reads the row)
    o.geo_row = (f.RVEL && f.geo && sub_h) ? f.geo + 8 * (long)sub_h[0] : nullptr;
    o.geo_stride = 8 * (long)f.n_h;
    o.nyquist = f.nyquist;
    o.sub_w0 = sub_w ? sub_w[0] : 0.0;
    o.var_u = f.var_u; o.var_v = f.var_v; o.var_w = f.var_w;
    o.n_rays = f.n_rays; o.n_gates = f.n_gates;
    o.with_attenuation = f.with_attenuation;
    o.c_zh = f.c_zh; o.c_kdp = f.c_kdp; o.c_2w = f.c_2w; o.res_km = f.res_km;
    return o;
}
