// Host check of the composite validation (cosmo_pol_amd/csrc/cpol_comp.h); tests/test_composite_cpu.py drives it.
//   comp_check CALL ...     the calls of one context in turn; the pass they open and close is kept between them.  One CALL:
//       key=value,... with rows gates space phase fields(hex) products rpb nx ny hlo hhi (either: a slab) rays(0: NULL
//       ray_sin) count(0: NULL) values(0: NULL) and, after ';', lists  x=e0:e1:...  y=e0:e1:...  ("x=null": NULL pointer) and
//       tK=t0:t1:...  (field K's thresholds; "nK=" overrides n_thresholds[K]) -- strtod syntax, so hex floats, nan and inf are taken
// prints one line per call:
//   refused <reason>
//   ok blocks B rpb R cells C zero Z state S begin b finish f open o slab s hlo H hhi H | field K slot S planes P max O count O top
//   O low O thr t0 t1 ... | x edges ... | y edges ...     (%a: exact)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "cpol_comp.h"

int main(int argc, char **argv)
{
    CompPass pass;
    static uint64_t count_sink[1];
    static float value_sink[1];
    static const double ray[1] = {0.0};
    for (int i = 1; i < argc; ++i) {
        std::string call = argv[i];
        std::map<std::string, std::string> kv;
        std::vector<double> ex, ey, thr[COMP_FIELDS];
        bool x_null = false, y_null = false, x_given = false, y_given = false;
        size_t semi = call.find(';');
        std::string head = call.substr(0, semi), tail = semi == std::string::npos ? "" : call.substr(semi + 1);
        for (size_t p = 0; p < head.size();) {
            size_t q = head.find(',', p);
            if (q == std::string::npos) q = head.size();
            const std::string item = head.substr(p, q - p);
            const size_t eq = item.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad item '%s'\n", item.c_str()); return 2; }
            kv[item.substr(0, eq)] = item.substr(eq + 1);
            p = q + 1;
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
            std::vector<double> *dst = nullptr;
            if (name == "x") { if (list == "null") { x_null = true; continue; } dst = &ex; x_given = true; }
            else if (name == "y") { if (list == "null") { y_null = true; continue; } dst = &ey; y_given = true; }
            else if (name[0] == 't') {
                const int k = atoi(name.c_str() + 1);
                if (k < 0 || k >= COMP_FIELDS) { fprintf(stderr, "bad field '%s'\n", name.c_str()); return 2; }
                dst = &thr[k];
            } else { fprintf(stderr, "bad list name '%s'\n", name.c_str()); return 2; }
            for (size_t a = 0; a < list.size();) {
                size_t b = list.find(':', a);
                if (b == std::string::npos) b = list.size();
                dst->push_back(strtod(list.substr(a, b - a).c_str(), nullptr));
                a = b + 1;
            }
        }
        const auto num = [&](const char *k, long dflt) { return kv.count(k) ? strtol(kv[k].c_str(), nullptr, 0) : dflt; };
        CompCall c;
        c.n_rows = num("rows", 1); c.n_gates = (int)num("gates", 1);
        c.spaceborne = num("space", 0) != 0;
        cpol_composite s;
        memset(&s, 0, sizeof s);
        s.fields = (uint32_t)num("fields", 1); s.phase = (int32_t)num("phase", 3); s.products = (uint32_t)num("products", 1);
        s.rays_per_block = (int32_t)num("rpb", 0);
        s.n_x = (int32_t)num("nx", x_given ? (long)ex.size() - 1 : (x_null ? 1 : 0));
        s.n_y = (int32_t)num("ny", y_given ? (long)ey.size() - 1 : (y_null ? 1 : 0));
        if (x_given) s.edges_x = ex.data();
        if (y_given) s.edges_y = ey.data();
        if (kv.count("hlo") || kv.count("hhi")) {
            s.use_slab = 1;
            s.h_lo = kv.count("hlo") ? strtod(kv["hlo"].c_str(), nullptr) : -HUGE_VAL;
            s.h_hi = kv.count("hhi") ? strtod(kv["hhi"].c_str(), nullptr) : HUGE_VAL;
        }
        if (num("rays", 1)) { s.ray_sin = ray; s.ray_cos = ray; }
        if (num("count", 1)) s.count = count_sink;
        for (int k = 0; k < COMP_FIELDS; ++k) {
            if (num("values", 1)) s.values[k] = value_sink;
            s.n_thresholds[k] = (int32_t)thr[k].size() > COMP_MAX_THR ? COMP_MAX_THR + 1 : (int32_t)thr[k].size();
            for (size_t j = 0; j < thr[k].size() && j < (size_t)COMP_MAX_THR; ++j) s.thresholds[k][j] = thr[k][j];
            char key[8];
            snprintf(key, sizeof key, "n%d", k);
            if (kv.count(key)) s.n_thresholds[k] = (int32_t)num(key, 0);
        }
        CompPlan pl;
        const char *why = comp_check(&s, c, pass, &pl);
        if (why) { printf("refused %s\n", why); continue; }
        comp_advance(&s, pl, &pass);
        printf("ok blocks %ld rpb %ld cells %ld zero %ld state %ld begin %d finish %d open %d slab %d hlo %a hhi %a", pl.n_blocks,
               pl.rows_per_block, pl.cells, pl.zero_bytes, pl.state_bytes, (int)pl.begin, (int)pl.finish, (int)pass.open, (int)pl.slab,
               (double)pl.h_lo, (double)pl.h_hi);
        for (int j = 0; j < pl.n_fields; ++j) {
            const int k = pl.field[j];
            printf(" | field %d slot %d planes %d max %ld count %ld top %ld low %ld thr", k, pl.slot[k], pl.n_planes[k], pl.off_max[k],
                   pl.off_count[k], pl.off_top[k], pl.off_low[k]);
            for (float t : pl.thr[k]) printf(" %a", (double)t);
        }
        printf(" | x edges"); for (double e : pl.ex) printf(" %a", e);
        printf(" | y edges"); for (double e : pl.ey) printf(" %a", e);
        printf("\n");
    }
    return 0;
}
