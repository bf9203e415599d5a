// Host check of the terrain-shadowing launch rule (cosmo_pol_amd/csrc/cpol_forms.h: FormIn.shadow); tests/test_terrain_shadow_cpu.py
// drives it.  Over a table of calls -- n_sub 1 / 3 / 4 / 49, n_rays 1 / 16 / 360, every entry point, Doppler 0-3, melting, lanes 0 / 2,
// three species sets, the knobs that pick the fused forms and the graph --
//   shadow = false: every field of Forms equals what a FormIn that never heard of the field (default-constructed) gives;
//   shadow = true:  fused, fused_gate1, present and graphable are false, the interpolation is a launch of its own wherever the
//                   entry point interpolates, and every decision of the second half of the sequence is the unshadowed call's.
// Prints SHADOW_FORMS_OK, the calls walked and how many of them lost a fused form, a presence word or the graph to the shadow.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "cpol_forms.h"

static void species(FormIn &in, const char *set)
{
    in.n_hydro = 0;
    for (const char *p = set; *p; ++p) {
        FormSpecies s;
        s.tab = true; s.n_pan = 64; s.pan_hi = 63; s.pre = s.dnu = true;
        s.psd_family = CPOL_PSD_GAMMA; s.q_source = CPOL_Q_MODEL; s.uniform_grid = 1;
        switch (*p) {
        case 'R': s.rule = CPOL_RULE_RAIN_1MOM; s.var_q = 3; break;
        case 'S': s.rule = CPOL_RULE_SNOW_1MOM; s.var_q = 4; s.uniform_grid = 0; break;
        case 'G': s.rule = CPOL_RULE_GRAUPEL_1MOM; s.var_q = 5; break;
        case 'm': s.psd_family = CPOL_PSD_MELTING; s.two_d = true; s.writes_vn = true; s.pre = s.dnu = false; s.tab_degree = CPOL_MELT_DEGREE;
                  s.rule = CPOL_RULE_MELTING_SNOW; s.q_source = CPOL_Q_MELT_SNOW; break;
        case 'x': s.rule = CPOL_RULE_GRAUPEL_1MOM; s.var_q = 5; s.tab = false; s.n_pan = s.pan_hi = 0; break;     // a slot without a table
        default: continue;
        }
        in.s[in.n_hydro++] = s;
    }
}

// every field of Forms, in declaration order
static std::vector<long> fields(const Forms &f)
{
    std::vector<long> v = {f.lanes, f.ray_prep, f.prep_paths, f.geo_poly, f.poly_single, f.traj_launch, f.traj_paths, f.melt_qr, f.melt_qs,
                           f.melt_qg, f.sub_melt, f.any_2d, f.all_tab, f.any_tab, f.subsum, f.final_inplace, f.gate1, f.fused_gate1,
                           f.by_species, f.gate1_ray, f.g1r, f.present};
    for (int j = 0; j < CPOL_MAX_HYDRO; ++j) v.push_back(f.vsrc[j]);
    const long rest[] = {f.any_vsrc2, f.rare_direct, f.fused, f.plain_interp, f.stencil, f.drop_latlon, f.want_szt, f.n_tiles, f.use_tile_list,
                         f.lookup_launch, f.lookup_tile, f.rare_fork, f.lookup_split, f.psd_need[0], f.psd_need[1], f.psd_need[2], f.psd_need[3],
                         f.psd_rare_one, f.psd_fork, f.psd_ice_tab, f.psd_melt_tab, f.psd_melt_direct, f.psd_modes, f.sum_form, f.sum_team,
                         f.sum_tile_log2, f.sum_chain, f.rvel_terms, f.final_512, f.graphable};
    v.insert(v.end(), rest, rest + sizeof rest / sizeof *rest);
    return v;
}

int main()
{
    const int subs[4] = {1, 3, 4, 49}, rays[3] = {1, 16, 360};
    const char *sets[3] = {"RSG", "RSGm", "RSx"};
    struct Entry { bool columns, sub_export, members, timed; } entries[5] = {
        {false, false, false, false}, {true, false, false, false}, {false, true, false, false}, {false, false, true, false}, {false, false, true, true}};
    long n = 0, lost = 0;
    for (int kn = 0; kn < 4; ++kn) {
        Knobs k;
        ProcessKnobs pk;
        if (kn == 1) k.use_graph = true;
        if (kn == 2) { k.fuse_gate1 = 1; k.use_graph = true; }
        if (kn == 3) { k.gate1_ray = 1; k.fuse_classify = 1; }
        for (int n_sub : subs) for (int n_rays : rays) for (const Entry &e : entries) for (int dop = 0; dop < 4; ++dop)
        for (int melt = 0; melt < 2; ++melt) for (int lanes = 0; lanes <= 2; lanes += 2) for (const char *sp : sets) for (int ml = 0; ml < 2; ++ml) {
            FormIn in;                                   // (default-constructed: shadow as the struct leaves it)
            in.n_rays = in.geo_rays = n_rays; in.n_gates = 170; in.n_sub = n_sub; in.n_h = n_sub > 1 ? 7 : 1; in.nz = 30; in.scan_form = 1;
            in.versioned = true; in.reuse = true; in.outputs_on_device = 1;
            in.columns = e.columns; in.sub_export = e.sub_export; in.members = e.members; in.timed = e.timed;
            in.doppler = dop; in.with_melting = melt != 0; in.lanes = lanes; in.ml = ml != 0;
            species(in, sp);
            const Forms base = choose_forms(in, k, pk);
            FormIn off = in;
            off.shadow = false;
            const Forms f0 = choose_forms(off, k, pk);
            FormIn on = in;
            on.shadow = true;
            const Forms f1 = choose_forms(on, k, pk);
            ++n;
            const char *bad = nullptr;
            if (fields(f0) != fields(base)) bad = "shadow = false changed a decision";
            int r0[12], rb[12];
            forms_record(off, f0, r0);
            forms_record(in, base, rb);
            if (!bad && memcmp(r0, rb, sizeof r0) != 0) bad = "shadow = false changed launch_forms";
            if (!bad && (f1.fused || f1.fused_gate1 || f1.present || f1.graphable)) bad = "shadow = true kept fused / fused_gate1 / present / graphable";
            if (!bad && !in.columns && !in.members && !f1.plain_interp) bad = "shadow = true: the interpolation is no launch of its own";
            if (!bad) {
                // the second half: what the unshadowed call decides, the four forms and what follows from them (plain_interp, stencil) aside
                Forms a = base, b = f1;
                a.fused = b.fused = a.fused_gate1 = b.fused_gate1 = a.present = b.present = a.graphable = b.graphable = false;
                a.plain_interp = b.plain_interp = a.stencil = b.stencil = false;
                // (CPOL_FUSE_GATE1=1: without k_interp_gate1 the single-beam kernel may take its one-wavefront-per-species form)
                if (base.fused_gate1) a.by_species = b.by_species = false;
                if (fields(a) != fields(b)) bad = "shadow = true changed a decision of the second half";
            }
            if (!bad && base.stencil && !f1.stencil) bad = "shadow = true lost the gate stencil";
            if (bad) {
                printf("%s (knobs %d, n_sub %d, n_rays %d, columns %d, export %d, members %d, timed %d, doppler %d, melting %d, lanes %d, species %s, ml %d)\n",
                       bad, kn, n_sub, n_rays, e.columns, e.sub_export, e.members, e.timed, dop, melt, lanes, sp, ml);
                return 1;
            }
            if (base.fused || base.fused_gate1 || base.present || base.graphable) ++lost;
        }
    }
    printf("SHADOW_FORMS_OK %ld %ld\n", n, lost);
    return 0;
}
