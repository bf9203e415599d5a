// Host check of the histogram validation (cosmo_pol_amd/csrc/cpol_hist.h); tests/test_histogram_cpu.py drives it.
//   hist_check CALL ...     the calls of one context in turn; the pass they open and close is kept between them.  One CALL:
//       key=value,... with rows gates dop nmv phase fields(hex) ord ny rpb counts(0: no counts pointers) and, after ';',
//       edge lists  xK=e0:e1:...  (field K's abscissa; "xK=null" leaves the pointer NULL) and  y=e0:e1:...  -- strtod syntax,
//       so hex floats, nan and inf are taken
// prints one line per call:
//   refused <reason>
//   ok blocks B rpb R state S begin b finish f open o | field K cells C off O edges e0 e1 ... | y edges ...     (%a: exact)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "cpol_hist.h"

int main(int argc, char **argv)
{
    HistPass pass;
    static uint64_t sink[1];
    for (int i = 1; i < argc; ++i) {
        std::string call = argv[i];
        std::map<std::string, std::string> kv;
        std::vector<double> ex[HIST_FIELDS], ey;
        bool x_null[HIST_FIELDS] = {}, x_given[HIST_FIELDS] = {}, y_given = false;
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
            if (eq == std::string::npos) { fprintf(stderr, "bad edge list '%s'\n", item.c_str()); return 2; }
            const std::string name = item.substr(0, eq), list = item.substr(eq + 1);
            std::vector<double> *dst = &ey;
            if (name[0] == 'x') {
                const int k = atoi(name.c_str() + 1);
                if (k < 0 || k >= HIST_FIELDS) { fprintf(stderr, "bad field '%s'\n", name.c_str()); return 2; }
                if (list == "null") { x_null[k] = true; continue; }
                dst = &ex[k]; x_given[k] = true;
            } else y_given = true;
            for (size_t a = 0; a < list.size();) {
                size_t b = list.find(':', a);
                if (b == std::string::npos) b = list.size();
                dst->push_back(strtod(list.substr(a, b - a).c_str(), nullptr));
                a = b + 1;
            }
        }
        const auto num = [&](const char *k, long dflt) { return kv.count(k) ? strtol(kv[k].c_str(), nullptr, 0) : dflt; };
        HistCall c;
        c.n_rows = num("rows", 1); c.n_gates = (int)num("gates", 1); c.doppler = num("dop", 1) != 0;
        c.n_model_vars = (int)num("nmv", 0);
        cpol_histogram h;
        memset(&h, 0, sizeof h);
        h.fields = (uint32_t)num("fields", 1); h.phase = (int32_t)num("phase", 3); h.ordinate = (int32_t)num("ord", 0);
        h.n_y = (int32_t)num("ny", y_given ? (long)ey.size() - 1 : 0); h.rays_per_block = (int32_t)num("rpb", 0);
        for (int k = 0; k < HIST_FIELDS; ++k) {
            if (x_given[k]) { h.n_x[k] = (int32_t)ex[k].size() - 1; h.edges_x[k] = ex[k].data(); }
            if (x_null[k]) h.n_x[k] = 1;
            char key[8];
            snprintf(key, sizeof key, "nx%d", k);
            if (kv.count(key)) h.n_x[k] = (int32_t)num(key, 0);         // (an n_x that the list does not back: the limits)
            if (num("counts", 1)) h.counts[k] = sink;
        }
        if (y_given) h.edges_y = ey.data();
        HistPlan pl;
        const char *why = hist_check(&h, c, pass, &pl);
        if (why) { printf("refused %s\n", why); continue; }
        hist_advance(&h, pl, &pass);
        printf("ok blocks %ld rpb %ld state %ld begin %d finish %d open %d", pl.n_blocks, pl.rows_per_block, pl.state_cells,
               (int)pl.begin, (int)pl.finish, (int)pass.open);
        for (int j = 0; j < pl.n_fields; ++j) {
            const int k = pl.field[j];
            printf(" | field %d cells %d off %ld edges", k, pl.cells[k], pl.state_off[k]);
            for (double e : pl.ex[k]) printf(" %a", e);
        }
        if (pl.n_ey) { printf(" | y edges"); for (double e : pl.ey) printf(" %a", e); }
        printf("\n");
    }
    return 0;
}
