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

#include "../../include/cosmo_pol_amd.h"      // (the CPOL_RULE_*, CPOL_PSD_* and CPOL_Q_* codes)

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

// ---- the operands of k_gate1_ray's ITEM phase, one record per hydrometeor slot (round 11) ----
// Every wavefront that holds items used to take what its species' rule and table position need out of HydroDev, ItabDev and
// ClassifyArgs one field at a time (classify_item, cpol_psd.inl: about 20 awaited scalar rounds on the rain / graupel path, three
// of them in front of the gate's three model values), and asked for its first coefficient rows only behind the item's scale
// and fall-speed moments -- three exponentials and four float64 divisions by species constants.  The record holds exactly
// what the gamma 1-moment rules (rain, snow, graupel) on a 1-D integral table read: the first 64-byte line what the value
// loads need, with vals + var * n resolved on the host; the other lines the rule, the table position and the Doppler
// constants, the quotients by nu already formed (IEEE division of the same operands in the same order: the bits of the
// device's).  Anything else is `generic`: the wavefront calls classify_item as before.  Filled at every launch; nothing is kept.
enum {
    CPOL_G1S_GENERIC = 1,       // the record does not cover the slot: classify_item
    CPOL_G1S_HAS_VN = 2,        // analytic fall-speed moments are formed (ClassifyArgs.doppler, gamma family, not numeric_intv)
    CPOL_G1S_WRITES_VN = 4,     // RVEL is asked for and the table carries the Doppler sums (ItabDev.writes_vn)
    CPOL_G1S_MOMENTS = 8,       // RVEL is asked for and the slot's moments enter it per gate (FinalArgs.vsrc[j] == 1)
    CPOL_G1S_N0_UNIFORM = 16,   // the intercept is the species' n0_fixed (rain, graupel): dv_pre, dn_pre hold
    CPOL_G1S_RVEL = 32          // RVEL is asked for
};
// (GENERIC says how the item is classified, nothing more: the pointers of the first line, the sweep's shape, w0 and the bits
// WRITES_VN, MOMENTS and RVEL hold for every slot of the launch, so that a wavefront of k_gate1_ray reads them in one place)

struct alignas(64) Gate1SpeciesOps {
    // line 0: the value loads (and what snow asks for as soon as T is in)
    const float *elev;
    const float *val_t;            // ClassifyArgs.vals + var_t * n_sbg
    const float *val_q;            // ClassifyArgs.vals + var_q * n_sbg
    const float *tfun_snow;        // or NULL
    const double *tab;             // the slot's 1-D integral table
    int n_rays, n_gates;
    int rule;
    int flags;                     // CPOL_G1S_*
    int key_base, n_pan;
    // line 1: bins, the rule and the position on the panel axis -- everything in front of the first coefficient request
    float e_lo, e_step, t_lo, t_step;
    float a32;                     // (float)a: the factor of snow's float32 chain
    int n_e, n_t;
    int ppo, pan_lo, pan_hi;
    double lambda_factor, lam_exponent, log2_lo;
    // line 2: the scale and the Doppler constants -- formed while the first rows travel
    double d0;
    double vn_exp_v;               // -(beta + mu + 1) / nu
    double vn_exp_n;               // -(mu + 1) / nu
    double dv_pre;                 // vel_factor * n0_fixed * alpha / nu    (n0_uniform)
    double dn_pre;                 // ntot_factor * n0_fixed / nu           (n0_uniform)
    double vel_factor, alpha, nu;  // (snow: its intercept is the lane's, it divides on the device)
    // line 3
    double ntot_factor;
    double w0;                     // sub_w[0]: the weight of the ONE sub-beam
    double n0_fixed, a;            // (as the descriptor has them: what dv_pre, dn_pre and a32 were formed from)
    int pad_[8];
};
static_assert(sizeof(Gate1SpeciesOps) % 64 == 0 && alignof(Gate1SpeciesOps) == 64, "the record arrives in whole 64-byte scalar loads");
static_assert(sizeof(Gate1SpeciesOps) == 256, "no hidden padding: 5 pointers, 6 ints | 5 floats, 5 ints, 3 doubles | 8 doubles | 4 doubles, 8 ints");
static_assert(offsetof(Gate1SpeciesOps, e_lo) == 64 && offsetof(Gate1SpeciesOps, d0) == 128 && offsetof(Gate1SpeciesOps, ntot_factor) == 192,
              "the value loads need the first line alone, the first coefficient request the first two");

// the records of a launch of k_gate1_ray: one per slot (a c2 launch fills 3); a wavefront loads only its own slot's lines
struct Gate1SpeciesSet {
    Gate1SpeciesOps s[CPOL_MAX_HYDRO];
};

// H: HydroDev, T: ItabDev, C: ClassifyArgs, F: FinalArgs (templates as above); j: the slot (FinalArgs.vsrc is per slot);
// sub_w: the HOST array of the sweep's sub-beam weights
template <class H, class T, class C, class F>
inline Gate1SpeciesOps gate1_species_ops(const H &h, const T &t, const C &c, const F &f, int j, const double *sub_w)
{
    Gate1SpeciesOps o{};
    const auto &d = h.d;
    const bool rule_ok = d.rule == CPOL_RULE_RAIN_1MOM || d.rule == CPOL_RULE_GRAUPEL_1MOM || d.rule == CPOL_RULE_SNOW_1MOM;
    const bool generic = !rule_ok || d.psd_family != CPOL_PSD_GAMMA || d.q_source != CPOL_Q_MODEL || d.second_axis_f64 || d.numeric_intv ||
                         !t.tab || t.two_d || t.par_slot != 0 || c.wgate || f.wgate || f.n_sub != 1 || !c.vals || !c.elev || !sub_w;
    const bool uniform = d.rule != CPOL_RULE_SNOW_1MOM;
    const bool want_rvel = f.RVEL != nullptr;
    o.flags = (generic ? CPOL_G1S_GENERIC : 0) | ((c.doppler && !generic) ? CPOL_G1S_HAS_VN : 0) | ((want_rvel && t.writes_vn) ? CPOL_G1S_WRITES_VN : 0) |
              ((want_rvel && f.vsrc[j] == 1) ? CPOL_G1S_MOMENTS : 0) | (uniform ? CPOL_G1S_N0_UNIFORM : 0) | (want_rvel ? CPOL_G1S_RVEL : 0);
    o.w0 = sub_w ? sub_w[0] : 0.0;
    o.elev = c.elev;
    o.val_t = c.vals ? c.vals + (long)d.var_t * c.n_sbg : nullptr;
    o.val_q = c.vals ? c.vals + (long)d.var_q * c.n_sbg : nullptr;
    o.tfun_snow = c.tfun_snow;
    o.tab = t.tab;
    o.n_rays = f.n_rays; o.n_gates = f.n_gates;
    o.rule = d.rule;
    o.key_base = h.key_base; o.n_pan = t.n_pan;
    o.e_lo = d.e_lo; o.e_step = d.e_step; o.t_lo = d.t_lo; o.t_step = d.t_step;
    o.n_e = d.n_e; o.n_t = d.n_t;
    o.ppo = t.ppo; o.pan_lo = t.pan_lo; o.pan_hi = t.pan_hi;
    o.lambda_factor = d.lambda_factor; o.lam_exponent = d.lam_exponent; o.n0_fixed = d.n0_fixed; o.a = d.a;
    o.a32 = (float)d.a;                                     // (classify_item: float an0 = (float)d.a * n0)
    o.log2_lo = t.log2_lo; o.d0 = t.d0;
    // (classify_item: dv = vel_factor * n0v * alpha / nu * exp(-(beta + mu + 1) / nu * lp), dn = ntot_factor * n0v / nu * exp(-(mu + 1) / nu * lp))
    o.vn_exp_v = -(d.beta + d.mu + 1) / d.nu;
    o.vn_exp_n = -(d.mu + 1) / d.nu;
    if (uniform) {
        o.dv_pre = d.vel_factor * d.n0_fixed * d.alpha / d.nu;
        o.dn_pre = d.ntot_factor * d.n0_fixed / d.nu;
    }
    o.vel_factor = d.vel_factor; o.alpha = d.alpha; o.nu = d.nu; o.ntot_factor = d.ntot_factor;
    return o;
}

// HS: HydroSet, IS: ItabSet: the records of a launch (no wavefront reads the record of a slot beyond the launch's species)
template <class HS, class IS, class C, class F>
inline Gate1SpeciesSet gate1_species_set(const HS &hs, const IS &its, const C &c, const F &f, const double *sub_w)
{
    Gate1SpeciesSet o{};
    for (int j = 0; j < CPOL_MAX_HYDRO; ++j) {
        if (j < hs.n_hydro) o.s[j] = gate1_species_ops(hs.h[j], its.t[j], c, f, j, sub_w);
        else o.s[j].flags = CPOL_G1S_GENERIC;
    }
    return o;
}
