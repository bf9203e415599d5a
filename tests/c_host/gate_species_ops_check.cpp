// Host check of the species record of cpol_gate_ops.h (tests/test_gate_species_ops_cpu.py): the record of k_gate1_ray's item
// phase equals its sources field by field for two slots that differ in every field, the resolved pointers are vals + var * n,
// every host-divided constant has the bits of classify_item's expression evaluated plainly, its size is a whole number of
// 64-byte lines, and `generic` is set for each excluded case alone and clear for rain, snow and graupel.
#include <cstdio>
#include <cstring>

#include "cpol_gate_ops.h"

// stand-ins with the field names of cpol_hydro_desc, HydroDev, ItabDev (cpol_device.h), ClassifyArgs (cpol_psd.inl) and
// FinalArgs (cpol_final.inl) that the filler reads
struct Desc {
    int psd_family, rule, q_source, var_q, var_t, n_e, n_t, second_axis_f64, numeric_intv;
    float e_lo, e_step, t_lo, t_step;
    double a, alpha, beta, mu, nu, lambda_factor, ntot_factor, vel_factor, n0_fixed, lam_exponent;
};
struct Hydro { Desc d; int key_base; };
struct Itab {
    const double *tab;
    double log2_lo, d0;
    int n_pan, pan_lo, pan_hi, writes_vn, ppo, two_d, par_slot;
};
struct Classify {
    float *vals;
    const float *elev, *tfun_snow;
    const double *wgate;
    long n_sbg;
    int doppler;
};
struct Final {
    double *RVEL;
    const double *wgate;
    int n_rays, n_gates, n_sub;
    int vsrc[CPOL_MAX_HYDRO];
};
struct HydroSetS { int n_hydro; Hydro h[CPOL_MAX_HYDRO]; };
struct ItabSetS { Itab t[CPOL_MAX_HYDRO]; };

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static float f32[4096];
static double f64[64];

static bool same_bits(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }

// the bench's 1-moment species (cosmo_pol_amd/hydrometeors.py _consts('R' | 'S' | 'G', '1mom') and the fixed intercepts) and
// sets that are no round numbers
struct Psd { double alpha, nu, beta, mu, vel_factor, ntot_factor, n0_fixed; };
static const Psd PSDS[] = {
    {4.110960958218893, 1.0, 0.5, 0.5, 1.0, 0.8862269254527579, 1253.029102860344},          // rain
    {0.8713569109190723, 1.0, 0.25, 0.0, 0.906402477055477, 1.0, 0.0},                       // snow: the intercept is the lane's
    {0.9449792435599864, 1.0, 0.89, 0.0, 0.9583793077186229, 1.0, 4000.0},                   // graupel
    {3.0, 3.0, 2.0 / 3.0, 1.0 / 3.0, 0.3333333333333333, 0.2975983731199, 1.0e6 / 7.0},     // nu != 1: every quotient rounds
    {0.1, 0.7, 1.9, -0.3, 1.7724538509055159, 2.6789385347077476, 12345.678},
};

static Hydro make_hydro(int k, int rule, const Psd &p)
{
    Hydro h{};
    Desc &d = h.d;
    d.psd_family = CPOL_PSD_GAMMA; d.rule = rule; d.q_source = CPOL_Q_MODEL;
    d.var_q = 3 + k; d.var_t = 1 + k; d.n_e = 8 + k; d.n_t = 20 + k;
    d.e_lo = 0.5f + k; d.e_step = 1.5f + k; d.t_lo = 200.0f + k; d.t_step = 2.5f + k;
    d.a = 0.038 + k; d.alpha = p.alpha; d.beta = p.beta; d.mu = p.mu; d.nu = p.nu;
    d.lambda_factor = 6.25 + k; d.ntot_factor = p.ntot_factor; d.vel_factor = p.vel_factor; d.n0_fixed = p.n0_fixed;
    d.lam_exponent = 0.25 + 0.125 * k;
    h.key_base = 160 * k + 7;
    return h;
}

static Itab make_itab(int k)
{
    Itab t{};
    t.tab = f64 + 1 + k; t.log2_lo = -3.5 + k; t.d0 = 0.2 + k;
    t.n_pan = 96 + k; t.pan_lo = 2 + k; t.pan_hi = 90 + k; t.ppo = 8 + 8 * k;
    t.writes_vn = 0; t.two_d = 0; t.par_slot = 0;
    return t;
}

static Classify make_classify(int k)
{
    Classify c{};
    c.vals = f32 + 5 + k; c.elev = f32 + 9 + k; c.tfun_snow = f32 + 13 + k;
    c.n_sbg = 350 + k; c.doppler = 1;
    return c;
}

static Final make_final(int k)
{
    Final f{};
    f.RVEL = f64 + 3 + k; f.n_rays = 5 + k; f.n_gates = 70 + k; f.n_sub = 1;
    for (int j = 0; j < CPOL_MAX_HYDRO; ++j) f.vsrc[j] = 1;
    return f;
}

static void check_fields(int k, int rule, const Psd &p)
{
    const Hydro h = make_hydro(k, rule, p);
    const Itab t = make_itab(k);
    const Classify c = make_classify(k);
    const Final f = make_final(k);
    const double sub_w[2] = {0.75 + k, 9.0};
    const Desc &d = h.d;
    const Gate1SpeciesOps o = gate1_species_ops(h, t, c, f, 2, sub_w);
    const bool uniform = rule != CPOL_RULE_SNOW_1MOM;
    CHECK(o.flags == (CPOL_G1S_HAS_VN | CPOL_G1S_MOMENTS | CPOL_G1S_RVEL | (uniform ? CPOL_G1S_N0_UNIFORM : 0)));
    CHECK(o.elev == c.elev && o.tfun_snow == c.tfun_snow && o.tab == t.tab);
    CHECK(o.val_t == c.vals + (long)d.var_t * c.n_sbg && o.val_q == c.vals + (long)d.var_q * c.n_sbg);
    CHECK(o.n_rays == f.n_rays && o.n_gates == f.n_gates && o.rule == d.rule && o.key_base == h.key_base && o.n_pan == t.n_pan);
    CHECK(o.e_lo == d.e_lo && o.e_step == d.e_step && o.t_lo == d.t_lo && o.t_step == d.t_step && o.a32 == (float)d.a);
    CHECK(o.n_e == d.n_e && o.n_t == d.n_t && o.ppo == t.ppo && o.pan_lo == t.pan_lo && o.pan_hi == t.pan_hi);
    CHECK(o.lambda_factor == d.lambda_factor && o.lam_exponent == d.lam_exponent && o.log2_lo == t.log2_lo && o.d0 == t.d0);
    CHECK(o.vel_factor == d.vel_factor && o.alpha == d.alpha && o.nu == d.nu && o.ntot_factor == d.ntot_factor);
    CHECK(o.n0_fixed == d.n0_fixed && o.a == d.a && o.w0 == sub_w[0]);
    for (int q = 0; q < (int)(sizeof o.pad_ / sizeof o.pad_[0]); ++q) CHECK(o.pad_[q] == 0);
    // the constants: classify_item's expressions, evaluated plainly on volatile operands (nothing folded at compile time)
    volatile double beta = d.beta, mu = d.mu, nu = d.nu, vel = d.vel_factor, ntot = d.ntot_factor, alpha = d.alpha, n0v = d.n0_fixed;
    CHECK(same_bits(o.vn_exp_v, -(beta + mu + 1) / nu));
    CHECK(same_bits(o.vn_exp_n, -(mu + 1) / nu));
    if (uniform) {
        CHECK(same_bits(o.dv_pre, vel * n0v * alpha / nu));
        CHECK(same_bits(o.dn_pre, ntot * n0v / nu));
    } else {
        CHECK(o.dv_pre == 0.0 && o.dn_pre == 0.0);
    }
}

static int generic_of(const Hydro &h, const Itab &t, const Classify &c, const Final &f, const double *sub_w)
{
    return gate1_species_ops(h, t, c, f, 0, sub_w).flags & CPOL_G1S_GENERIC;
}

int main()
{
    CHECK(sizeof(Gate1SpeciesOps) % 64 == 0 && alignof(Gate1SpeciesOps) == 64 && sizeof(Gate1SpeciesSet) == CPOL_MAX_HYDRO * sizeof(Gate1SpeciesOps));
    const int rules[3] = {CPOL_RULE_RAIN_1MOM, CPOL_RULE_SNOW_1MOM, CPOL_RULE_GRAUPEL_1MOM};
    for (int k = 0; k < 2; ++k)                    // (every source value of k = 1 differs from k = 0's: no field is checked against a constant)
        for (int r = 0; r < 3; ++r)
            for (const Psd &p : PSDS) check_fields(k, rules[r], p);
    // ---- generic: clear for the three rules, set by each excluded case alone
    const double sub_w[1] = {1.0};
    const Classify c0 = make_classify(0);
    const Final f0 = make_final(0);
    const Itab t0 = make_itab(0);
    for (int r = 0; r < 3; ++r) CHECK(generic_of(make_hydro(0, rules[r], PSDS[r]), t0, c0, f0, sub_w) == 0);
    {
        const int others[4] = {CPOL_RULE_TWO_MOMENT, CPOL_RULE_ICE_1MOM, CPOL_RULE_MELTING_SNOW, CPOL_RULE_MELTING_GRAUPEL};
        for (int r = 0; r < 4; ++r) CHECK(generic_of(make_hydro(0, others[r], PSDS[0]), t0, c0, f0, sub_w) != 0);
        Hydro h = make_hydro(0, rules[0], PSDS[0]);
        h.d.psd_family = CPOL_PSD_ICE_FIELD; CHECK(generic_of(h, t0, c0, f0, sub_w) != 0);
        h = make_hydro(0, rules[0], PSDS[0]); h.d.q_source = CPOL_Q_MELT_SNOW; CHECK(generic_of(h, t0, c0, f0, sub_w) != 0);
        h = make_hydro(0, rules[0], PSDS[0]); h.d.second_axis_f64 = 1; CHECK(generic_of(h, t0, c0, f0, sub_w) != 0);
        h = make_hydro(0, rules[0], PSDS[0]); h.d.numeric_intv = 1; CHECK(generic_of(h, t0, c0, f0, sub_w) != 0);
        h = make_hydro(0, rules[0], PSDS[0]);
        Itab t = t0; t.tab = nullptr; CHECK(generic_of(h, t, c0, f0, sub_w) != 0);
        t = t0; t.two_d = 1; CHECK(generic_of(h, t, c0, f0, sub_w) != 0);
        t = t0; t.par_slot = 2; CHECK(generic_of(h, t, c0, f0, sub_w) != 0);
        Classify c = c0; c.wgate = f64; CHECK(generic_of(h, t0, c, f0, sub_w) != 0);
        Final f = f0; f.wgate = f64; CHECK(generic_of(h, t0, c0, f, sub_w) != 0);
        f = f0; f.n_sub = 2; CHECK(generic_of(h, t0, c0, f, sub_w) != 0);
        CHECK(generic_of(h, t0, c0, f0, nullptr) != 0);
        // and nothing else: no RVEL, no Doppler, the table carrying the sums, another moment source
        f = f0; f.RVEL = nullptr; c = c0; c.doppler = 0; c.tfun_snow = nullptr; t = t0; t.writes_vn = 1;
        const Gate1SpeciesOps o = gate1_species_ops(h, t, c, f, 0, sub_w);
        CHECK(o.flags == CPOL_G1S_N0_UNIFORM);
        f = f0; f.vsrc[0] = 2;
        CHECK(gate1_species_ops(h, t, c0, f, 0, sub_w).flags == (CPOL_G1S_HAS_VN | CPOL_G1S_WRITES_VN | CPOL_G1S_RVEL | CPOL_G1S_N0_UNIFORM));
        // a generic record still carries what every wavefront reads in one place
        h.d.numeric_intv = 1;
        const Gate1SpeciesOps g = gate1_species_ops(h, t0, c0, f0, 0, sub_w);
        CHECK(g.flags == (CPOL_G1S_GENERIC | CPOL_G1S_MOMENTS | CPOL_G1S_RVEL | CPOL_G1S_N0_UNIFORM));
        CHECK(g.n_rays == f0.n_rays && g.n_gates == f0.n_gates && g.elev == c0.elev && g.w0 == sub_w[0]);
        CHECK(g.val_t == c0.vals + (long)h.d.var_t * c0.n_sbg && g.val_q == c0.vals + (long)h.d.var_q * c0.n_sbg);
    }
    // ---- the set of a launch: one record per slot of the launch, slot j's from slot j's sources
    {
        HydroSetS hs{};
        ItabSetS its{};
        hs.n_hydro = 3;
        for (int j = 0; j < 3; ++j) { hs.h[j] = make_hydro(j & 1, rules[j], PSDS[j]); hs.h[j].key_base = 100 * j; its.t[j] = make_itab(j & 1); }
        Final f = f0;
        f.vsrc[1] = 2;
        const Gate1SpeciesSet s = gate1_species_set(hs, its, c0, f, sub_w);
        for (int j = 0; j < 3; ++j) {
            CHECK(s.s[j].key_base == 100 * j && s.s[j].rule == rules[j] && !(s.s[j].flags & CPOL_G1S_GENERIC));
            CHECK(((s.s[j].flags & CPOL_G1S_MOMENTS) != 0) == (j != 1));
        }
        for (int j = 3; j < CPOL_MAX_HYDRO; ++j) CHECK(s.s[j].flags == CPOL_G1S_GENERIC && s.s[j].tab == nullptr);
    }
    if (fails) return 1;
    std::printf("GATE_SPECIES_OPS_OK %zu bytes\n", sizeof(Gate1SpeciesOps));
    return 0;
}
