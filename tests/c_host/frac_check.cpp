// Host check of the neighbourhood-verification validation (cosmo_pol_amd/csrc/cpol_frac.h); tests/test_neighbourhood_cpu.py
// drives it.
//   frac_check CALL ...     independent calls.  One CALL: key=value,... -- of the composite beside it: comp(0: none) cphase
//       cfields(hex) cproducts ctop(echo-top thresholds per field) nx ny rows rpb; of the cpol_fractions: field plane obs(0: NULL)
//       sums(0: NULL) totals(0: NULL) dom(1: given) nthr / nrad (override the counts) -- and, after ';', lists  t=t0:t1:...
//       (thresholds) and  r=r0:r1:...  (radii); strtod syntax, so hex floats, nan and inf are taken
// prints one line per call:
//   composite refused <reason>
//   refused <reason>
//   ok blocks B cells C table T tables N scratch S field K first F stride P rows R cols C score S chunks H groups G sums X totals Y
//   | thr t0 ... | radii r0 ...     (%a: exact)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "cpol_frac.h"

int main(int argc, char **argv)
{
    static uint64_t count_sink[1], sums_sink[1], totals_sink[1];
    static float value_sink[1], obs_sink[1];
    static uint8_t dom_sink[1];
    static const double ray[1] = {0.0};
    for (int i = 1; i < argc; ++i) {
        std::string call = argv[i];
        std::map<std::string, std::string> kv;
        std::vector<double> thr, rad;
        size_t semi = call.find(';');
        std::string head = call.substr(0, semi), tail = semi == std::string::npos ? "" : call.substr(semi + 1);
        for (size_t p = 0; p < head.size();) {
            size_t q = head.find(',', p);
            if (q == std::string::npos) q = head.size();
            const std::string item = head.substr(p, q - p);
            p = q + 1;
            if (item.empty()) continue;
            const size_t eq = item.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad item '%s'\n", item.c_str()); return 2; }
            kv[item.substr(0, eq)] = item.substr(eq + 1);
        }
        for (size_t p = 0; p < tail.size();) {
            size_t q = tail.find(';', p);
            if (q == std::string::npos) q = tail.size();
            const std::string item = tail.substr(p, q - p);
            p = q + 1;
            if (item.empty()) continue;
            const size_t eq = item.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad list '%s'\n", item.c_str()); return 2; }
            const std::string name = item.substr(0, eq), list = item.substr(eq + 1);
            std::vector<double> *dst = name == "t" ? &thr : name == "r" ? &rad : nullptr;
            if (!dst) { fprintf(stderr, "bad list name '%s'\n", name.c_str()); return 2; }
            for (size_t a = 0; a < list.size();) {
                size_t b = list.find(':', a);
                if (b == std::string::npos) b = list.size();
                dst->push_back(strtod(list.substr(a, b - a).c_str(), nullptr));
                a = b + 1;
            }
        }
        const auto num = [&](const char *k, long dflt) { return kv.count(k) ? strtol(kv[k].c_str(), nullptr, 0) : dflt; };
        // the composite of the call: a grid of nx x ny unit cells
        const int nx = (int)num("nx", 3), ny = (int)num("ny", 2);
        std::vector<double> ex((size_t)(nx > 0 ? nx : 0) + 1), ey((size_t)(ny > 0 ? ny : 0) + 1);
        for (size_t j = 0; j < ex.size(); ++j) ex[j] = (double)j;
        for (size_t j = 0; j < ey.size(); ++j) ey[j] = (double)j;
        CompCall cc;
        cc.n_rows = num("rows", 4); cc.n_gates = 5;
        cpol_composite c;
        memset(&c, 0, sizeof c);
        c.fields = (uint32_t)num("cfields", 1); c.phase = (int32_t)num("cphase", 3); c.products = (uint32_t)num("cproducts", 1);
        c.rays_per_block = (int32_t)num("rpb", 0);
        c.n_x = nx; c.n_y = ny; c.edges_x = ex.data(); c.edges_y = ey.data();
        c.ray_sin = ray; c.ray_cos = ray; c.count = count_sink;
        for (int k = 0; k < COMP_FIELDS; ++k) {
            c.values[k] = value_sink;
            c.n_thresholds[k] = (c.products & CPOL_COMP_ECHO_TOP) ? (int32_t)num("ctop", 1) : 0;
            for (int j = 0; j < c.n_thresholds[k] && j < COMP_MAX_THR; ++j) c.thresholds[k][j] = 1.0 + j;
        }
        const bool with_comp = num("comp", 1) != 0;
        CompPass pass;
        CompPlan cpl;
        if (with_comp) {
            const char *why = comp_check(&c, cc, pass, &cpl);
            if (why) { printf("composite refused %s\n", why); continue; }
        }
        cpol_fractions f;
        memset(&f, 0, sizeof f);
        f.field = (int32_t)num("field", 0); f.plane = (int32_t)num("plane", 0);
        f.n_thresholds = (int32_t)(kv.count("nthr") ? num("nthr", 0) : (long)thr.size());
        f.n_radii = (int32_t)(kv.count("nrad") ? num("nrad", 0) : (long)rad.size());
        for (size_t j = 0; j < thr.size() && j < (size_t)FRAC_MAX_THR; ++j) f.thresholds[j] = thr[j];
        for (size_t j = 0; j < rad.size() && j < (size_t)FRAC_MAX_RADII; ++j) f.radii[j] = (int32_t)rad[j];
        if (num("obs", 1)) f.observed = obs_sink;
        if (num("dom", 0)) f.domain = dom_sink;
        if (num("sums", 1)) f.sums = sums_sink;
        if (num("totals", 1)) f.totals = totals_sink;
        FracPlan pl;
        const char *why = frac_check(&f, with_comp ? &c : nullptr, with_comp ? &cpl : nullptr, &pl);
        if (why) { printf("refused %s\n", why); continue; }
        printf("ok blocks %ld cells %ld table %ld tables %ld scratch %ld field %d first %ld stride %ld rows %ld cols %ld score %ld chunks %d "
               "groups %d sums %zu totals %zu | thr", pl.n_blocks, pl.cells, pl.table, pl.n_tables, pl.scratch_bytes, pl.field, pl.plane_first,
               pl.plane_stride, pl.grid_rows, pl.grid_cols, pl.grid_score, pl.col_chunks, pl.score_groups, pl.sums_bytes, pl.totals_bytes);
        for (int j = 0; j < pl.n_thr; ++j) printf(" %a", (double)pl.thr[j]);
        printf(" | radii");
        for (int j = 0; j < pl.n_radii; ++j) printf(" %d", pl.radii[j]);
        printf("\n");
    }
    return 0;
}
