// Host check of the work-buffer plan (cosmo_pol_amd/csrc/cpol_buffers.h); tests/test_buffers_cpu.py drives it and holds every
// expected value.  Each command writes int64 records to <file>: what plan_buffers was given (with the Forms choose_forms made of
// the call) and what it returned.
//   buffers_check walk <file>      the enumerated space: shapes x species counts x variables x Doppler / broadening x 'ml' x debug
//                                  reads x entry points, then the knob sets of forms_check.cpp over the shapes and entry points
//   buffers_check columns <file>   the columns call with host and device inputs and every set of optional inputs; wide records
//   buffers_check big <file>       2^31 - 1 sub-beam gates with CPOL_MAX_HYDRO species; wide records
//   buffers_check table            the rows of BUF_ROWS as text, and buf_per_gate for every (n_hydro, n_vars)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "cpol_buffers.h"

// species as forms_check.cpp names them: R S G (1-moment gamma species on 1-D tables), mS mG (melting: 2-D tables), I (1-moment
// ice), N (2-moment, numeric fall-speed sums); a trailing '-': no integral table
static void species_of(const std::string &name, FormSpecies &s)
{
    std::string n = name;
    const bool untab = !n.empty() && n.back() == '-';
    if (untab) n.pop_back();
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
    } else { s.rule = CPOL_RULE_TWO_MOMENT; s.var_q = 6; s.numeric_intv = 1; s.writes_vn = true; }       // "N"
    if (untab) { s.tab = s.two_d = false; s.n_pan = s.pan_hi = 0; }
}

static void set_species(FormIn &in, const std::vector<std::string> &names)
{
    in.n_hydro = (int)names.size();
    for (int j = 0; j < in.n_hydro; ++j) species_of(names[j], in.s[j]);
}

enum Entry { E_SWEEP, E_MEMBERS, E_TIMED, E_EXPORT, E_COLUMNS, E_COLUMNS_DEV, E_COLUMNS_MELT, E_N };

static void set_entry(FormIn &in, int e)
{
    in.columns = e >= E_COLUMNS; in.sub_export = e == E_EXPORT; in.members = e == E_MEMBERS || e == E_TIMED; in.timed = e == E_TIMED;
    in.melt_given = e == E_COLUMNS_MELT;
}

struct Extra {                         // what run_sequence adds to the Forms' input
    int n_v = 1, n_vars = 9, n_keys = 0, n_vbins = 0;
    bool broaden = false, inputs_on_device = false, present_words = false;
    int classify_threads = 256;
    bool col_given[6] = {true, true, false, false, false, false};
};

static FILE *out = nullptr;
static long n_records = 0;

static void emit(const FormIn &in, const Knobs &k, const ProcessKnobs &pk, const Extra &x, int tag, bool wide)
{
    BufIn bi;
    bi.n_rays = in.n_rays; bi.n_gates = in.n_gates; bi.n_sub = in.n_sub; bi.n_h = in.n_h; bi.n_v = x.n_v; bi.n_vars = x.n_vars;
    bi.n_hydro = in.n_hydro; bi.n_keys = x.n_keys; bi.n_vbins = x.n_vbins; bi.mode = in.geometry_mode;
    bi.keep_debug = in.keep_debug; bi.ml = in.ml; bi.doppler = in.doppler != 0; bi.dop3 = in.doppler == 3; bi.broaden = x.broaden;
    bi.timed = in.timed; bi.columns = in.columns; bi.inputs_on_device = x.inputs_on_device; bi.sub_export = in.sub_export;
    for (int q = 0; q < 6; ++q) bi.col_given[q] = in.columns && x.col_given[q];
    bi.classify_threads = x.classify_threads; bi.present_words = x.present_words;
    bi.f = choose_forms(in, k, pk);
    const BufPlan pl = plan_buffers(bi);
    const Forms &f = bi.f;
    int key[WB_N];
    const int n_key = buf_key_list(pl, key);
    int64_t key_mask = 0;
    for (int q = 0; q < n_key; ++q) key_mask |= (int64_t)1 << key[q];
    int64_t given = 0;
    for (int q = 0; q < 6; ++q) given |= (int64_t)bi.col_given[q] << q;
    std::vector<int64_t> r = {
        bi.n_rays, bi.n_gates, bi.n_sub, bi.n_h, bi.n_v, bi.n_vars, bi.n_hydro, bi.n_keys, bi.n_vbins, bi.mode,
        (int64_t)bi.keep_debug | (int64_t)bi.ml << 1 | (int64_t)bi.doppler << 2 | (int64_t)bi.dop3 << 3 | (int64_t)bi.broaden << 4 |
            (int64_t)bi.timed << 5 | (int64_t)bi.columns << 6 | (int64_t)bi.inputs_on_device << 7 | (int64_t)bi.sub_export << 8 |
            (int64_t)bi.present_words << 9 | given << 10,
        bi.classify_threads,
        (int64_t)f.ray_prep | (int64_t)f.prep_paths << 1 | (int64_t)f.geo_poly << 2 | (int64_t)f.rvel_terms << 3 | (int64_t)f.gate1 << 4 |
            (int64_t)f.gate1_ray << 5 | (int64_t)f.rare_direct << 6 | (int64_t)f.subsum << 7 | (int64_t)f.graphable << 8,
        f.g1r, tag};
    for (int w = 0; w < WB_N; ++w) r.push_back((int64_t)pl.bytes[w]);
    const int64_t tail[11] = {pl.cnt_stride, pl.unit_cap, (int64_t)pl.xscr_mask, (int64_t)pl.xscr_elev, (int64_t)pl.xgeo_lons, (int64_t)pl.xgeo_dist,
                              (int64_t)pl.xgeo_heights, (int64_t)pl.xgeo_elev, (int64_t)pl.xgeo_mlmask, key_mask, pl.n_col};
    r.insert(r.end(), tail, tail + 11);
    if (wide) {
        for (int q = 0; q < BUF_MAX_COLS; ++q) r.push_back((int64_t)pl.col_bytes[q]);
        for (int q = 0; q < BUF_MAX_COLS; ++q) r.push_back((int64_t)pl.col_off[q]);
    }
    fwrite(r.data(), sizeof(int64_t), r.size(), out);
    ++n_records;
}

static const int RAYS[3] = {1, 3, 257}, GATES[4] = {1, 64, 65, 513}, SUBS[4] = {1, 3, FORMS_RAY_PREP_MIN_SUB, 49};
static const char *const SPECIES[CPOL_MAX_HYDRO] = {"R", "S", "G", "I", "N", "mS", "mG", "R"};

static void shape(FormIn &in, Extra &x, int n_rays, int ng, int n_sub)
{
    in.n_rays = in.geo_rays = n_rays; in.n_gates = ng; in.n_sub = n_sub;
    in.n_h = n_sub >= 49 ? 7 : n_sub >= 3 ? 3 : 1;
    x.n_v = n_sub >= 49 ? 7 : n_sub >= 4 ? 2 : 1;
    x.n_keys = 40 * in.n_hydro + 1;
}

static void flags(FormIn &in, Extra &x, int dop, bool broaden, bool ml, bool dbg)
{
    in.doppler = dop; x.broaden = broaden; x.n_vbins = dop == 3 ? 64 : 0; in.ml = ml; in.keep_debug = dbg;
    x.col_given[2] = ml;
    for (int q = 3; q < 6; ++q) x.col_given[q] = in.melt_given;
}

// the whole shape space on the default knobs, with lanes alive (k_gate1_ray where the rules allow it)
// (<file> "-": the records to the standard output, their number to the standard error)
static void walk_shapes()
{
    FormIn in;
    in.nz = 80; in.scan_form = 1; in.versioned = true; in.reuse = true; in.outputs_on_device = 1; in.lanes = 2;
    const Knobs k0;
    const ProcessKnobs p0;
    Knobs kg = k0;
    kg.use_graph = true;
    const int vars[3] = {1, 9, CPOL_MAX_VARS}, entries[5] = {E_SWEEP, E_MEMBERS, E_TIMED, E_EXPORT, E_COLUMNS};
    for (int n_hyd = 1; n_hyd <= CPOL_MAX_HYDRO; ++n_hyd) {
        set_species(in, std::vector<std::string>(SPECIES, SPECIES + n_hyd));
        for (int n_rays : RAYS) for (int ng : GATES) for (int n_sub : SUBS) for (int n_vars : vars) for (int e : entries)
        for (int dop = 0; dop < 4; ++dop) for (int br = 0; br < 2; ++br) for (int ml = 0; ml < 2; ++ml) for (int dbg = 0; dbg < 2; ++dbg) {
            Extra x;
            x.n_vars = n_vars;
            set_entry(in, e);
            shape(in, x, n_rays, ng, n_sub);
            flags(in, x, dop, br != 0, ml != 0, dbg != 0);
            emit(in, e == E_SWEEP ? kg : k0, p0, x, 0, false);          // (the sweeps with CPOL_USE_GRAPH=1: the graphable ones)
        }
    }
}

// the knob sets of forms_check.cpp (cmd_implications), each over the shapes, the entry points and forms_check's species sets
static int tag_next = 1;

static void walk_knobs(FormIn in, const Knobs &k, const ProcessKnobs &pk, Extra x)
{
    const std::vector<std::string> sets[3] = {{"R", "S", "G"}, {"R", "S", "G", "mS"}, {"R", "S-", "G"}};
    const int tag = tag_next++;
    // (lanes alive throughout: without them the default of CPOL_GATE1_RAY decides what its value 0 decides, which is walked)
    for (int n_rays : RAYS) for (int ng : {1, 65}) for (int n_sub : SUBS) for (int e = 0; e < E_N; ++e) for (int dbg = 0; dbg < 2; ++dbg)
    for (int dop = 0; dop < 4; ++dop) for (const auto &sp : sets) {
        const int n_h = in.n_h;
        set_species(in, sp);
        set_entry(in, e);
        shape(in, x, n_rays, ng, n_sub);
        if (n_h > 1) in.n_h = n_h;                       // (the geometry modes walk three horizontal nodes)
        flags(in, x, dop, dop == 3 && dbg, in.ml, dbg != 0);
        x.inputs_on_device = e == E_COLUMNS_DEV;
        in.lanes = 2;
        emit(in, k, pk, x, tag, false);
        in.n_h = n_h;
    }
}

static void walk_knob_sets()
{
    FormIn in;
    in.n_h = 1; in.nz = 80; in.scan_form = 1; in.versioned = true; in.reuse = true; in.outputs_on_device = 1;
    const Knobs k0;
    const ProcessKnobs p0;
    const Extra x0;
    walk_knobs(in, k0, p0, x0);
    struct { int Knobs::*m; int v[5]; int n; } ints[] = {
        {&Knobs::subsum_coop_rounds, {0, 64}, 2}, {&Knobs::rare_overlap, {1}, 1}, {&Knobs::rare_direct, {0}, 1}, {&Knobs::lookup_list, {0, 2}, 2},
        {&Knobs::lookup_split, {1, 16}, 2}, {&Knobs::gate1_ray, {0, 1, 2, 3}, 4}, {&Knobs::gate1_species, {0, 2}, 2}, {&Knobs::fuse_gate1, {1}, 1},
        {&Knobs::fuse_classify, {0}, 1}, {&Knobs::gate1, {0, 2}, 2}, {&Knobs::subsum, {0}, 1}, {&Knobs::subsum_scalar, {1}, 1},
        {&Knobs::upload_kernel, {1}, 1}, {&Knobs::geo_poly_central, {0, 2}, 2}, {&Knobs::geo_poly, {0}, 1}, {&Knobs::psd_rare, {0}, 1},
        {&Knobs::subsum_small, {1}, 1}, {&Knobs::subsum_chain, {0}, 1}, {&Knobs::subsum_team, {0, 2, 4, 8}, 4}, {&Knobs::subsum_coop, {0, 1}, 2}};
    for (const auto &c : ints)
        for (int q = 0; q < c.n; ++q) {
            Knobs k = k0;
            k.*(c.m) = c.v[q];
            walk_knobs(in, k, p0, x0);
        }
    Knobs kg = k0;
    kg.use_graph = true;
    walk_knobs(in, kg, p0, x0);
    {
        Knobs k = kg;
        k.fuse_gate1 = 1; k.gate1_ray = 1;
        walk_knobs(in, k, p0, x0);
        k = kg;
        k.gate1_ray = 3;                                 // (the tickets of the rays under a graph)
        walk_knobs(in, k, p0, x0);
    }
    ProcessKnobs p = p0;
    p.gate1_present = 0; p.exp_skip = 7; p.lookup_tile = 0; p.psd_only = 5; p.psd_siblings = true; p.final_512 = 1;
    walk_knobs(in, k0, p, x0);
    struct { bool FormIn::*m; bool v; } fl[] = {
        {&FormIn::ml, true}, {&FormIn::site, true}, {&FormIn::versioned, false}, {&FormIn::exact_sub, true}, {&FormIn::want_latlon, true},
        {&FormIn::want_sz_total, true}, {&FormIn::want_model, true}, {&FormIn::reuse, false}, {&FormIn::skip_melting, true}};
    for (const auto &c : fl) {
        FormIn i2 = in;
        i2.*(c.m) = c.v;
        walk_knobs(i2, k0, p0, x0);
        walk_knobs(i2, kg, p0, x0);
    }
    for (int mode = 1; mode <= 2; ++mode) {
        FormIn i2 = in;
        i2.geometry_mode = mode; i2.site = mode == CPOL_GEOM_SPACEBORNE; i2.n_h = 3;
        walk_knobs(i2, k0, p0, x0);
        walk_knobs(i2, kg, p0, x0);
    }
    {
        FormIn i2 = in;
        i2.nz = 32768; i2.timing = 2; i2.outputs_on_device = 2;
        walk_knobs(i2, k0, p0, x0);
        walk_knobs(i2, kg, p0, x0);
    }
    // the build constants of the kernel files that run_sequence hands in: a build with the presence words, another classify workgroup
    Extra x = x0;
    x.present_words = true; x.classify_threads = 512;
    Knobs k = kg;
    k.gate1_ray = 1;
    walk_knobs(in, k, p0, x);
}

static void walk_columns()
{
    FormIn in;
    in.nz = 80; in.scan_form = 1; in.versioned = true; in.reuse = true;
    set_species(in, {"R", "S", "G", "mS"});
    set_entry(in, E_COLUMNS);
    const Knobs k0;
    const ProcessKnobs p0;
    const int vars[3] = {1, 9, CPOL_MAX_VARS};
    for (int n_rays : RAYS) for (int ng : GATES) for (int n_sub : SUBS) for (int n_vars : vars) for (int dev = 0; dev < 2; ++dev)
    for (int given = 0; given < 64; ++given) {
        Extra x;
        x.n_vars = n_vars; x.inputs_on_device = dev != 0;
        shape(in, x, n_rays, ng, n_sub);
        for (int q = 0; q < 6; ++q) x.col_given[q] = (given >> q) & 1;
        in.ml = x.col_given[2]; in.melt_given = x.col_given[3];
        emit(in, k0, p0, x, given, true);
    }
}

static void walk_big()
{
    FormIn in;
    in.nz = 80; in.scan_form = 1; in.versioned = true; in.reuse = true; in.lanes = 2;
    set_species(in, std::vector<std::string>(SPECIES, SPECIES + CPOL_MAX_HYDRO));
    const Knobs k0;
    const ProcessKnobs p0;
    for (int e = 0; e < E_N; ++e) for (int dbg = 0; dbg < 2; ++dbg) for (int dop = 0; dop < 4; ++dop) {
        Extra x;
        x.n_vars = CPOL_MAX_VARS;
        set_entry(in, e);
        in.n_rays = in.geo_rays = 1; in.n_gates = 2147483647; in.n_sub = 1; in.n_h = 1;
        x.n_keys = 1024 * 31;
        flags(in, x, dop, dop == 3, true, dbg != 0);
        if (dop == 3) x.n_vbins = 4097;
        x.inputs_on_device = e == E_COLUMNS_DEV;
        emit(in, k0, p0, x, e, true);
    }
}

static int cmd_table()
{
    for (int w = 0; w < WB_N; ++w) {
        const BufRow &r = BUF_ROWS[w];
        printf("row %d %d %d %d %d %d %d\n", w, r.gate, r.per_var, r.per_hyd, (int)r.per_gate, (int)r.held, (int)r.fill);
    }
    for (int n_hyd = 1; n_hyd <= CPOL_MAX_HYDRO; ++n_hyd)
        for (int n_vars = 1; n_vars <= CPOL_MAX_VARS; ++n_vars) printf("per_gate %d %d %zu\n", n_hyd, n_vars, buf_per_gate((size_t)n_vars, (size_t)n_hyd));
    printf("consts %d %d %d %d %d %d\n", (int)WB_N, CPOL_MAX_HYDRO, CPOL_MAX_VARS, FORMS_RAY_PREP_MIN_SUB, CPOL_N_SZ, BUF_MAX_COLS);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "table")) return cmd_table();
    if (argc != 3) { fprintf(stderr, "usage: buffers_check walk|columns|big <file> | table\n"); return 2; }
    out = strcmp(argv[2], "-") ? fopen(argv[2], "wb") : stdout;
    if (!out) { perror(argv[2]); return 2; }
    if (!strcmp(argv[1], "walk")) { walk_shapes(); walk_knob_sets(); }
    else if (!strcmp(argv[1], "columns")) walk_columns();
    else if (!strcmp(argv[1], "big")) walk_big();
    else return 2;
    if (fclose(out) != 0) return 2;
    fprintf(stderr, "BUFFERS_RECORDS %ld\n", n_records);
    return 0;
}
