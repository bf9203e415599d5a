// Host check of the launch rules (cosmo_pol_amd/csrc/cpol_forms.h); tests/test_forms_cpu.py drives it.
//   forms_check forms key=value ...   one call described on the command line, its context knobs taken from the environment
//                                     (knobs_from_env, process_knobs): prints the 12 launch_forms entries and the other decisions
//   forms_check knobs                 prints knobs_from_env() and process_knobs() as name=value
//   forms_check implications          walks a reduced input space and checks the implications run_sequence relies on; prints
//                                     FORMS_IMPLICATIONS_OK and the number of calls walked
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "cpol_forms.h"

// species by the names the bench and the tests use: R S G (1-moment gamma species on 1-D tables that kept every panel), mS mG
// (melting: 2-D tables), I (1-moment ice: a 1-D table, fall-speed sums over the ray), N (2-moment gamma species with numeric
// fall-speed sums); a trailing '-': no integral table, '~': a table that lost its upper panels to the accuracy gate
static bool species_of(const std::string &name, FormSpecies &s)
{
    std::string n = name;
    const char mod = !n.empty() && (n.back() == '-' || n.back() == '~') ? n.back() : 0;
    if (mod) n.pop_back();
    s = FormSpecies();
    s.tab = true; s.n_pan = 64; s.pan_hi = 63; s.pre = s.dnu = true;
    s.psd_family = CPOL_PSD_GAMMA; s.q_source = CPOL_Q_MODEL; s.uniform_grid = 1;
    if (n == "R") { s.rule = CPOL_RULE_RAIN_1MOM; s.var_q = 3; }
    else if (n == "S") { s.rule = CPOL_RULE_SNOW_1MOM; s.var_q = 4; s.uniform_grid = 0; }
    else if (n == "G") { s.rule = CPOL_RULE_GRAUPEL_1MOM; s.var_q = 5; }
    else if (n == "mS" || n == "mG") {
        s.psd_family = CPOL_PSD_MELTING; s.two_d = true; s.writes_vn = true; s.pre = s.dnu = false; s.tab_degree = CPOL_MELT_DEGREE;
        s.rule = n == "mS" ? CPOL_RULE_MELTING_SNOW : CPOL_RULE_MELTING_GRAUPEL;
        s.q_source = n == "mS" ? CPOL_Q_MELT_SNOW : CPOL_Q_MELT_GRAUPEL;
    } else if (n == "I") {
        s.psd_family = CPOL_PSD_ICE_FIELD; s.rule = CPOL_RULE_ICE_1MOM; s.var_q = 6; s.writes_vn = true; s.pre = s.dnu = false;
        s.tab_degree = CPOL_ICE_DEGREE;
    } else if (n == "N") { s.rule = CPOL_RULE_TWO_MOMENT; s.var_q = 6; s.numeric_intv = 1; s.writes_vn = true; }
    else return false;
    if (mod == '-') { s.tab = s.two_d = false; s.n_pan = s.pan_hi = 0; }
    if (mod == '~') s.pan_hi = 40;
    return true;
}

static bool set_species(FormIn &in, const char *list)
{
    in.n_hydro = 0;
    for (const char *p = list; *p;) {
        const char *e = strchr(p, ',');
        const std::string name = e ? std::string(p, e) : std::string(p);
        if (in.n_hydro >= CPOL_MAX_HYDRO || !species_of(name, in.s[in.n_hydro++])) return false;
        p = e ? e + 1 : p + name.size();
    }
    return in.n_hydro > 0;
}

static bool set_entry(FormIn &in, const std::string &e)
{
    in.columns = in.sub_export = in.members = in.timed = in.melt_given = false;
    if (e == "sweep") return true;
    if (e == "columns") { in.columns = true; return true; }
    if (e == "columns_melt") { in.columns = in.melt_given = true; return true; }
    if (e == "export") { in.sub_export = true; return true; }
    if (e == "members") { in.members = true; return true; }
    if (e == "timed") { in.members = in.timed = true; return true; }
    return false;
}

static int cmd_forms(int argc, char **argv)
{
    FormIn in;
    in.n_rays = 360; in.n_gates = 500; in.n_sub = 1; in.n_h = 1; in.nz = 80; in.scan_form = 1;
    in.versioned = true; in.reuse = true;
    set_species(in, "R,S,G");
    for (int a = 2; a < argc; ++a) {
        const char *eq = strchr(argv[a], '=');
        if (!eq) { fprintf(stderr, "not key=value: %s\n", argv[a]); return 2; }
        const std::string k((const char *)argv[a], eq), v(eq + 1);
        const int i = atoi(v.c_str());
        if (k == "n_rays") in.n_rays = i; else if (k == "n_gates") in.n_gates = i; else if (k == "n_sub") in.n_sub = i;
        else if (k == "n_h") in.n_h = i; else if (k == "mode") in.geometry_mode = i; else if (k == "doppler") in.doppler = i;
        else if (k == "ml") in.ml = i; else if (k == "skip_melting") in.skip_melting = i; else if (k == "site") in.site = i;
        else if (k == "versioned") in.versioned = i; else if (k == "with_melting") in.with_melting = i; else if (k == "exact") in.exact_sub = i;
        else if (k == "want_latlon") in.want_latlon = i; else if (k == "sz_total") in.want_sz_total = i; else if (k == "model") in.want_model = i;
        else if (k == "reuse") in.reuse = i; else if (k == "dev") in.outputs_on_device = i; else if (k == "debug") in.keep_debug = i;
        else if (k == "timing") in.timing = i; else if (k == "lanes") in.lanes = i; else if (k == "nz") in.nz = i;
        else if (k == "entry") { if (!set_entry(in, v)) { fprintf(stderr, "bad entry %s\n", v.c_str()); return 2; } }
        else if (k == "species") { if (!set_species(in, v.c_str())) { fprintf(stderr, "bad species %s\n", v.c_str()); return 2; } }
        else { fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
    }
    in.geo_rays = in.n_rays;
    const Forms f = choose_forms(in, knobs_from_env(), process_knobs());
    int rec[12];
    forms_record(in, f, rec);
    // (Context.FORM_NAMES of cosmo_pol_amd/_native.py, in its order)
    const char *names[12] = {"g1r", "gate1_ray", "gate1", "interp_classify", "rare_direct", "subbeam_sum", "final_inplace", "poly_central",
                             "n_sub", "lanes_alive", "scan_form", "graph_replayed"};
    for (int q = 0; q < 12; ++q) printf("%s=%d\n", names[q], rec[q]);
    printf("by_species=%d\nfused_gate1=%d\nstencil=%d\ngraphable=%d\nsum_form=%d\nsum_team=%d\nfinal_512=%d\nlookup_launch=%d\n"
           "psd_rare_one=%d\npsd_modes=%d\nmelt_qr=%d\nmelt_qs=%d\nmelt_qg=%d\nplain_interp=%d\nsum_chain=%d\nrvel_terms=%d\n",
           (int)f.by_species, (int)f.fused_gate1, (int)f.stencil, (int)f.graphable, f.sum_form, f.sum_team, (int)f.final_512, (int)f.lookup_launch,
           (int)f.psd_rare_one, f.psd_modes, f.melt_qr, f.melt_qs, f.melt_qg, (int)f.plain_interp, (int)f.sum_chain, (int)f.rvel_terms);
    return 0;
}

static int cmd_knobs()
{
    const Knobs k = knobs_from_env();
    const ProcessKnobs &p = process_knobs();
    printf("use_graph=%d\nsubsum_coop_rounds=%d\nrare_overlap=%d\nrare_direct=%d\nlookup_list=%d\nlookup_split=%d\ngate1_ray=%d\n"
           "gate1_species=%d\nfuse_gate1=%d\nfuse_classify=%d\ngate1=%d\nsubsum=%d\nsubsum_scalar=%d\nupload_kernel=%d\n"
           "geo_poly_central=%d\ngeo_poly=%d\npsd_rare=%d\nsubsum_small=%d\nsubsum_chain=%d\nsubsum_team=%d\nsubsum_coop=%d\n",
           (int)k.use_graph, k.subsum_coop_rounds, k.rare_overlap, k.rare_direct, k.lookup_list, k.lookup_split, k.gate1_ray,
           k.gate1_species, k.fuse_gate1, k.fuse_classify, k.gate1, k.subsum, k.subsum_scalar, k.upload_kernel,
           k.geo_poly_central, k.geo_poly, k.psd_rare, k.subsum_small, k.subsum_chain, k.subsum_team, k.subsum_coop);
    printf("p.gate1_present=%d\np.exp_skip=%d\np.lookup_tile=%d\np.lookup_fill=%ld\np.ice_force_sum=%d\np.psd_only=%d\np.psd_grid=%ld\n"
           "p.psd_grid_generic=%ld\np.psd_siblings=%d\np.psd_lds_pad=%ld\np.final_512=%d\n",
           p.gate1_present, p.exp_skip, p.lookup_tile, p.lookup_fill, p.ice_force_sum, p.psd_only, p.psd_grid,
           p.psd_grid_generic, (int)p.psd_siblings, p.psd_lds_pad, p.final_512);
    return 0;
}

// ---- the implications (tests/test_forms_cpu.py names the lines of run_sequence each one comes from) ----
static long n_calls = 0;

#define IMPLIES(a, b) do { if ((a) && !(b)) return #a " without " #b; } while (0)

static const char *broken(const FormIn &in, const Knobs &k, const Forms &f)
{
    bool all_tab = true;
    for (int j = 0; j < in.n_hydro; ++j) all_tab = all_tab && in.s[j].tab;
    const bool other_entry = in.columns || in.sub_export || in.members;
    IMPLIES(f.gate1, in.n_sub == 1 && f.final_inplace && f.rare_direct);
    IMPLIES(f.gate1_ray, f.gate1 && !in.with_melting && in.doppler != 2 && in.n_rays <= 65535);
    IMPLIES(f.gate1_ray, f.by_species);
    IMPLIES(f.by_species, f.gate1 && !f.fused_gate1);
    IMPLIES(f.fused_gate1, f.gate1 && !in.columns && !in.members);
    IMPLIES(f.present, f.gate1_ray && !in.columns && !in.members);
    IMPLIES(f.fused, f.rare_direct && !f.gate1 && !other_entry);
    IMPLIES(f.subsum, in.n_sub >= 4);
    IMPLIES(f.final_inplace && !f.gate1, in.n_sub < 4);
    IMPLIES(f.subsum, !f.final_inplace);
    IMPLIES(f.rare_direct, all_tab);
    IMPLIES(in.doppler == 3, !f.gate1 && !f.subsum && !f.fused && !f.rvel_terms);
    IMPLIES(f.poly_single, in.n_sub < FORMS_RAY_PREP_MIN_SUB && !in.columns && in.geometry_mode == CPOL_GEOM_GROUND_43 && !in.site && in.versioned);
    IMPLIES(f.geo_poly, f.ray_prep && !f.poly_single);
    IMPLIES(f.stencil, !k.use_graph && !f.graphable && in.nz < 32768 && in.n_sub == 1 && f.plain_interp);
    IMPLIES(f.graphable, !other_entry && in.doppler != 3 && k.use_graph);
    IMPLIES(f.plain_interp, !f.fused && !f.fused_gate1 && !in.columns && !in.members);
    IMPLIES(f.psd_rare_one, f.rare_direct);
    IMPLIES(f.rare_fork, f.lookup_launch && !f.gate1);
    IMPLIES(f.use_tile_list, f.rare_direct && !f.gate1);
    return nullptr;
}

static int walk_knobs(FormIn &in, const Knobs &k, const ProcessKnobs &pk, const char *what)
{
    const int subs[3] = {1, 3, 4}, rays[5] = {1, 15, 16, 300, 70000}, gates[3] = {1, 64, 65};
    const char *entries[6] = {"sweep", "columns", "columns_melt", "export", "members", "timed"};
    const char *sets[3] = {"R,S,G", "R,S,G,mS", "R,S-,G"};
    for (int n_sub : subs) for (int n_rays : rays) for (int ng : gates) for (const char *e : entries) for (int dbg = 0; dbg < 2; ++dbg)
    for (int dop = 0; dop < 4; ++dop) for (int melt = 0; melt < 2; ++melt) for (int lanes = 0; lanes <= 2; lanes += 2) for (const char *sp : sets) {
        in.n_sub = n_sub; in.n_rays = in.geo_rays = n_rays; in.n_gates = ng; in.keep_debug = dbg != 0; in.doppler = dop;
        in.with_melting = melt != 0; in.lanes = lanes;
        set_entry(in, e);
        set_species(in, sp);
        const Forms f = choose_forms(in, k, pk);
        ++n_calls;
        const char *bad = broken(in, k, f);
        if (bad) {
            printf("%s: %s (n_sub %d, n_rays %d, n_gates %d, entry %s, debug %d, doppler %d, melting %d, lanes %d, species %s)\n",
                   what, bad, n_sub, n_rays, ng, e, dbg, dop, melt, lanes, sp);
            return 1;
        }
    }
    return 0;
}

static int cmd_implications()
{
    FormIn in;
    in.n_h = 1; in.nz = 80; in.scan_form = 1; in.versioned = true; in.reuse = true; in.outputs_on_device = 1;
    const Knobs k0;
    const ProcessKnobs p0;
    if (walk_knobs(in, k0, p0, "defaults")) return 1;
    // every context knob at every documented value, one at a time
    struct { const char *name; int Knobs::*m; int v[5]; int n; } ints[] = {
        {"subsum_coop_rounds", &Knobs::subsum_coop_rounds, {0, 64}, 2}, {"rare_overlap", &Knobs::rare_overlap, {1}, 1},
        {"rare_direct", &Knobs::rare_direct, {0}, 1}, {"lookup_list", &Knobs::lookup_list, {0, 2}, 2},
        {"lookup_split", &Knobs::lookup_split, {1, 16}, 2}, {"gate1_ray", &Knobs::gate1_ray, {0, 1, 2, 3}, 4},
        {"gate1_species", &Knobs::gate1_species, {0, 2}, 2}, {"fuse_gate1", &Knobs::fuse_gate1, {1}, 1},
        {"fuse_classify", &Knobs::fuse_classify, {0}, 1}, {"gate1", &Knobs::gate1, {0, 2}, 2}, {"subsum", &Knobs::subsum, {0}, 1},
        {"subsum_scalar", &Knobs::subsum_scalar, {1}, 1}, {"upload_kernel", &Knobs::upload_kernel, {1}, 1},
        {"geo_poly_central", &Knobs::geo_poly_central, {0, 2}, 2}, {"geo_poly", &Knobs::geo_poly, {0}, 1}, {"psd_rare", &Knobs::psd_rare, {0}, 1},
        {"subsum_small", &Knobs::subsum_small, {1}, 1}, {"subsum_chain", &Knobs::subsum_chain, {0}, 1},
        {"subsum_team", &Knobs::subsum_team, {0, 2, 4, 8}, 4}, {"subsum_coop", &Knobs::subsum_coop, {0, 1}, 2}};
    for (const auto &c : ints)
        for (int q = 0; q < c.n; ++q) {
            Knobs k = k0;
            k.*(c.m) = c.v[q];
            if (walk_knobs(in, k, p0, c.name)) return 1;
        }
    {
        Knobs k = k0;
        k.use_graph = true;
        if (walk_knobs(in, k, p0, "use_graph")) return 1;
        k.fuse_gate1 = 1; k.gate1_ray = 1;                   // (the two single-beam fusions asked for together)
        if (walk_knobs(in, k, p0, "use_graph + fuse_gate1 + gate1_ray")) return 1;
    }
    // ... every process knob, and the inputs the walk holds fixed
    ProcessKnobs p = p0;
    p.gate1_present = 0; p.exp_skip = 7; p.lookup_tile = 0; p.psd_only = 5; p.psd_siblings = true; p.final_512 = 1;
    if (walk_knobs(in, k0, p, "process knobs")) return 1;
    struct { const char *name; bool FormIn::*m; bool v; } flags[] = {
        {"ml", &FormIn::ml, true}, {"site", &FormIn::site, true}, {"versioned", &FormIn::versioned, false}, {"exact_sub", &FormIn::exact_sub, true},
        {"want_latlon", &FormIn::want_latlon, true}, {"want_sz_total", &FormIn::want_sz_total, true}, {"want_model", &FormIn::want_model, true},
        {"reuse", &FormIn::reuse, false}, {"skip_melting", &FormIn::skip_melting, true}};
    Knobs kg = k0;
    kg.use_graph = true;
    for (const auto &c : flags) {
        FormIn i2 = in;
        i2.*(c.m) = c.v;
        if (walk_knobs(i2, k0, p0, c.name) || walk_knobs(i2, kg, p0, c.name)) return 1;
    }
    for (int mode = 1; mode <= 2; ++mode) {
        FormIn i2 = in;
        i2.geometry_mode = mode; i2.site = mode == CPOL_GEOM_SPACEBORNE; i2.n_h = 3;
        if (walk_knobs(i2, k0, p0, "geometry_mode") || walk_knobs(i2, kg, p0, "geometry_mode")) return 1;
    }
    {
        FormIn i2 = in;
        i2.nz = 32768; i2.timing = 2; i2.outputs_on_device = 2;
        if (walk_knobs(i2, k0, p0, "nz / timing / pinned outputs") || walk_knobs(i2, kg, p0, "nz / timing / pinned outputs")) return 1;
    }
    printf("FORMS_IMPLICATIONS_OK %ld\n", n_calls);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "forms")) return cmd_forms(argc, argv);
    if (argc == 2 && !strcmp(argv[1], "knobs")) return cmd_knobs();
    if (argc == 2 && !strcmp(argv[1], "implications")) return cmd_implications();
    fprintf(stderr, "usage: forms_check forms key=value ... | knobs | implications\n");
    return 2;
}
