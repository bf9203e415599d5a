// Host check of what the hydrometeor contributions add to the host-only rules (cpol_forms.h: FormIn::want_species; cpol_buffers.h:
// BufIn::want_species; cpol_products.h: PRODUCT_SPECIES); tests/test_species_rules_cpu.py drives it.
//   species_check forms          walks the FormIn grid of forms_check.cpp under the context knobs that reach the single-beam forms and
//                                prints  SPECIES_FORMS_OK <calls> <calls whose plain form takes a single-beam kernel>
//   species_check digest         prints a 64-bit FNV-1a digest of every decision of choose_forms over that grid WITHOUT the flag
//                                (built with -DSPECIES_CHECK_PARENT it compiles against a cpol_forms.h that has no such field)
//   species_check buffers        prints  SPECIES_BUFFERS_OK <plans>
//   species_check product ENTRY SET ...   as products_check, with `species` among the pointer names
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "cpol_buffers.h"
#ifndef SPECIES_CHECK_PARENT
#include "cpol_products.h"
#endif

// (the species of forms_check.cpp, by the same names)
static void species_of(const std::string &n, FormSpecies &s)
{
    s = FormSpecies();
    s.tab = true; s.n_pan = 64; s.pan_hi = 63; s.pre = s.dnu = true;
    s.psd_family = CPOL_PSD_GAMMA; s.q_source = CPOL_Q_MODEL; s.uniform_grid = 1;
    if (n == "R") { s.rule = CPOL_RULE_RAIN_1MOM; s.var_q = 3; }
    else if (n == "S" || n == "S-") { s.rule = CPOL_RULE_SNOW_1MOM; s.var_q = 4; s.uniform_grid = 0; }
    else if (n == "G") { s.rule = CPOL_RULE_GRAUPEL_1MOM; s.var_q = 5; }
    else if (n == "mS") {
        s.psd_family = CPOL_PSD_MELTING; s.two_d = true; s.writes_vn = true; s.pre = s.dnu = false; s.tab_degree = CPOL_MELT_DEGREE;
        s.rule = CPOL_RULE_MELTING_SNOW; s.q_source = CPOL_Q_MELT_SNOW;
    }
    if (n == "S-") { s.tab = s.two_d = false; s.n_pan = s.pan_hi = 0; }
}

static void set_species(FormIn &in, int which)
{
    static const char *const sets[3][4] = {{"R", "S", "G", nullptr}, {"R", "S", "G", "mS"}, {"R", "S-", "G", nullptr}};
    in.n_hydro = 0;
    for (int q = 0; q < 4 && sets[which][q]; ++q) species_of(sets[which][q], in.s[in.n_hydro++]);
}

static void set_entry(FormIn &in, int e)     // sweep, columns, columns_melt, export, members, timed
{
    in.columns = e == 1 || e == 2; in.melt_given = e == 2; in.sub_export = e == 3; in.members = e == 4 || e == 5; in.timed = e == 5;
}

// every decision of choose_forms, one number each, in the order of struct Forms
constexpr int D_GATE1 = 16, D_FUSED_GATE1 = 17, D_BY_SPECIES = 18, D_GATE1_RAY = 19, D_GRAPHABLE = 59, D_N = 60;
static int decisions(const Forms &f, long out[64])
{
    int n = 0;
    const auto put = [&](long v) { out[n++] = v; };
    put(f.lanes); put(f.ray_prep); put(f.prep_paths); put(f.geo_poly); put(f.poly_single); put(f.traj_launch); put(f.traj_paths);
    put(f.melt_qr); put(f.melt_qs); put(f.melt_qg); put(f.sub_melt); put(f.any_2d); put(f.all_tab); put(f.any_tab);
    put(f.subsum); put(f.final_inplace); put(f.gate1); put(f.fused_gate1); put(f.by_species); put(f.gate1_ray); put(f.g1r); put(f.present);
    for (int j = 0; j < CPOL_MAX_HYDRO; ++j) put(f.vsrc[j]);
    put(f.any_vsrc2); put(f.rare_direct); put(f.fused); put(f.plain_interp); put(f.stencil); put(f.drop_latlon); put(f.want_szt);
    put(f.n_tiles); put(f.use_tile_list); put(f.lookup_launch); put(f.lookup_tile); put(f.rare_fork); put(f.lookup_split);
    for (int m = 0; m < 4; ++m) put(f.psd_need[m]);
    put(f.psd_rare_one); put(f.psd_fork); put(f.psd_ice_tab); put(f.psd_melt_tab); put(f.psd_melt_direct); put(f.psd_modes);
    put(f.sum_form); put(f.sum_team); put(f.sum_tile_log2); put(f.sum_chain); put(f.rvel_terms); put(f.final_512); put(f.graphable);
    if (n != D_N) { fprintf(stderr, "decisions: %d entries\n", n); exit(3); }
    return n;
}

static long n_calls = 0;
[[maybe_unused]] static long n_fast = 0;
static unsigned long long digest = 1469598103934665603ull;

// the grid of forms_check.cpp's walk (its `implications`), under one set of knobs; check(in, k) per call
template <class Check>
static int walk(FormIn in, const Knobs &k, const char *what, Check check)
{
    const int subs[3] = {1, 3, 4}, rays[5] = {1, 15, 16, 300, 70000}, gates[3] = {1, 64, 65};
    for (int n_sub : subs) for (int n_rays : rays) for (int ng : gates) for (int e = 0; e < 6; ++e) for (int dbg = 0; dbg < 2; ++dbg)
    for (int dop = 0; dop < 4; ++dop) for (int melt = 0; melt < 2; ++melt) for (int lanes = 0; lanes <= 2; lanes += 2) for (int sp = 0; sp < 3; ++sp) {
        in.n_sub = n_sub; in.n_rays = in.geo_rays = n_rays; in.n_gates = ng; in.keep_debug = dbg != 0; in.doppler = dop;
        in.with_melting = melt != 0; in.lanes = lanes;
        set_entry(in, e);
        set_species(in, sp);
        ++n_calls;
        const char *bad = check(in, k);
        if (bad) {
            printf("%s: %s (n_sub %d, n_rays %d, n_gates %d, entry %d, debug %d, doppler %d, melting %d, lanes %d, species set %d)\n",
                   what, bad, n_sub, n_rays, ng, e, dbg, dop, melt, lanes, sp);
            return 1;
        }
    }
    return 0;
}

template <class Check>
static int walk_all(Check check)
{
    FormIn in;
    in.n_h = 1; in.nz = 80; in.scan_form = 1; in.versioned = true; in.reuse = true; in.outputs_on_device = 1;
    Knobs k;
    if (walk(in, k, "defaults", check)) return 1;
    k.use_graph = true;
    if (walk(in, k, "use_graph", check)) return 1;
    k.fuse_gate1 = 1; k.gate1_ray = 1;
    if (walk(in, k, "use_graph + fuse_gate1 + gate1_ray", check)) return 1;
    k = Knobs(); k.gate1 = 2;
    if (walk(in, k, "gate1 = 2", check)) return 1;
    k = Knobs(); k.gate1_ray = 3; k.gate1_species = 2;
    if (walk(in, k, "gate1_ray = 3, gate1_species = 2", check)) return 1;
    k = Knobs(); k.gate1 = 0;
    if (walk(in, k, "gate1 = 0", check)) return 1;
    k = Knobs(); k.fuse_classify = 0; k.rare_direct = 0;
    if (walk(in, k, "fuse_classify = 0, rare_direct = 0", check)) return 1;
    in.want_latlon = true; in.want_model = true;
    if (walk(in, Knobs(), "want_latlon + want_model", check)) return 1;
    return 0;
}

static const char *digest_call(const FormIn &in, const Knobs &k)
{
    long d[64];
    const int n = decisions(choose_forms(in, k, ProcessKnobs()), d);
    for (int q = 0; q < n; ++q)
        for (int b = 0; b < 8; ++b) { digest ^= (unsigned long long)((d[q] >> (8 * b)) & 0xff); digest *= 1099511628211ull; }
    return nullptr;
}

#ifndef SPECIES_CHECK_PARENT
static const char *forms_call(const FormIn &in, const Knobs &k)
{
    const ProcessKnobs pk;
    FormIn with = in;
    with.want_species = true;
    Knobs k0 = k;
    k0.gate1 = 0;                                  // CPOL_GATE1=0: the general launch sequence of the same call
    long plain[64], got[64], general[64];
    const int n = decisions(choose_forms(in, k, pk), plain);
    decisions(choose_forms(with, k, pk), got);
    decisions(choose_forms(in, k0, pk), general);
    // none of the four single-beam forms, no graph replay
    if (got[D_GATE1] || got[D_FUSED_GATE1] || got[D_BY_SPECIES] || got[D_GATE1_RAY]) return "a single-beam form with want_species";
    if (got[D_GRAPHABLE]) return "graphable with want_species";
    // a call whose plain form takes no single-beam kernel: nothing but graphable moves
    if (!plain[D_GATE1])
        for (int q = 0; q < n; ++q)
            if (q != D_GRAPHABLE && got[q] != plain[q]) return "want_species moves a decision of a call without single-beam forms";
    // every call: the decisions are those of the general sequence (what CPOL_GATE1=0 gives the plain call), graphable apart
    for (int q = 0; q < n; ++q)
        if (q != D_GRAPHABLE && got[q] != general[q]) return "want_species differs from the general launch sequence";
    // ... and the flag left at its default is no flag at all
    FormIn off = in;
    off.want_species = false;
    long again[64];
    decisions(choose_forms(off, k, pk), again);
    if (memcmp(again, plain, n * sizeof(long)) != 0) return "want_species = false differs from the default";
    n_fast += plain[D_GATE1] != 0;
    return nullptr;
}

static int cmd_buffers()
{
    long plans = 0;
    const int subs[3] = {1, 3, 9}, hyd[3] = {1, 3, 6};
    for (int n_sub : subs) for (int n_hyd : hyd) for (int dbg = 0; dbg < 2; ++dbg) for (int want = 0; want < 2; ++want) {
        FormIn in;
        in.n_rays = 5; in.n_gates = 70; in.n_sub = n_sub; in.n_h = 1; in.geo_rays = 5; in.nz = 80; in.versioned = true; in.keep_debug = dbg != 0;
        in.n_hydro = n_hyd;
        for (int j = 0; j < n_hyd; ++j) species_of(j == 0 ? "R" : j == 1 ? "S" : "G", in.s[j]);
        in.want_species = want != 0;
        BufIn bi;
        bi.n_rays = 5; bi.n_gates = 70; bi.n_sub = n_sub; bi.n_h = 1; bi.n_v = 1; bi.n_vars = 9; bi.n_hydro = n_hyd; bi.n_keys = 40;
        bi.keep_debug = dbg != 0; bi.classify_threads = 256; bi.present_words = true;
        bi.f = choose_forms(in, Knobs(), ProcessKnobs());
        BufIn with = bi;
        with.want_species = want != 0;
        const BufPlan a = plan_buffers(bi), b = plan_buffers(with);
        const size_t rows = (size_t)5 * 70 * n_hyd * CPOL_N_SZ * sizeof(float);
        const bool others = dbg || bi.f.subsum;
        if (a.bytes[WB_SZINTEG] != (others ? rows : 0)) { printf("plain: WB_SZINTEG %zu\n", a.bytes[WB_SZINTEG]); return 1; }
        if (b.bytes[WB_SZINTEG] != ((others || want) ? rows : 0)) { printf("want_species %d: WB_SZINTEG %zu\n", want, b.bytes[WB_SZINTEG]); return 1; }
        for (int w = 0; w < WB_N; ++w)
            if (w != WB_SZINTEG && a.bytes[w] != b.bytes[w]) { printf("want_species moves work buffer %d\n", w); return 1; }
        if (a.cnt_stride != b.cnt_stride || a.unit_cap != b.unit_cap) { printf("want_species moves the counters\n"); return 1; }
        ++plans;
    }
    printf("SPECIES_BUFFERS_OK %ld\n", plans);
    return 0;
}

static int cmd_product(int argc, char **argv)
{
    static const char *const entries[] = {"sweep", "members", "timed", "columns"};
    static const char *const products[] = {"none", "superob", "member_stats", "spectrum_moments", "histogram", "composite", "species"};
    int entry = -1;
    for (int e = 0; e < 4 && argc > 2; ++e)
        if (!strcmp(argv[2], entries[e])) entry = e;
    if (entry < 0) return 2;
    static cpol_superob so; static cpol_member_stats ms; static cpol_member_verify mv; static cpol_spectrum_moments sm;
    static cpol_histogram hg; static cpol_composite cp; static cpol_fractions fr; static cpol_species sp;
    for (int i = 3; i < argc; ++i) {
        cpol_outputs o;
        memset(&o, 0, sizeof o);
        const std::string set = std::string(",") + argv[i] + ",";
        const auto has = [&](const char *name) { return set.find(std::string(",") + name + ",") != std::string::npos; };
        if (has("superob")) o.superob = &so;
        if (has("member_stats")) o.member_stats = &ms;
        if (has("member_verify")) o.member_verify = &mv;
        if (has("spectrum_moments")) o.spectrum_moments = &sm;
        if (has("histogram")) o.histogram = &hg;
        if (has("composite")) o.composite = &cp;
        if (has("fractions")) o.fractions = &fr;
        if (has("species")) o.species = &sp;
        const CallProduct r = call_product(entry, o);
        if (r.refuse && r.refuse_after_plan) { fprintf(stderr, "two refusals for '%s'\n", argv[i]); return 1; }
        const char *const when = r.refuse ? (r.at_entry ? "entry" : "before") : r.refuse_after_plan ? "after" : "accepted";
        const char *const text = r.refuse ? r.refuse : r.refuse_after_plan ? r.refuse_after_plan : "-";
        printf("%s\t%s\t%s\n", products[r.product], when, text);
    }
    return 0;
}
#endif

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "digest")) {
        if (walk_all(digest_call)) return 1;
        printf("SPECIES_DIGEST %016llx %ld\n", digest, n_calls);
        return 0;
    }
#ifndef SPECIES_CHECK_PARENT
    if (argc == 2 && !strcmp(argv[1], "forms")) {
        if (walk_all(forms_call)) return 1;
        printf("SPECIES_FORMS_OK %ld %ld\n", n_calls, n_fast);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "buffers")) return cmd_buffers();
    if (argc >= 3 && !strcmp(argv[1], "product")) return cmd_product(argc, argv);
#endif
    fprintf(stderr, "usage: species_check forms | digest | buffers | product ENTRY SET ...\n");
    return 2;
}
