// Host check of the EXACT SUMS in the composite validation (cosmo_pol_amd/csrc/cpol_comp.h: the tail of a cpol_composite_sums, its
// refusals, the bins and skipped words of the state, the 1 GiB limit with them, the gates a block of a pass may fold);
// tests/test_composite_sums_cpu.py drives it.  comp_check.cpp, comp_check_network.cpp and comp_check_layers.cpp cover everything else.
//   comp_check_sums CALL ...   the calls of one context in turn; the pass they open and close is kept between them.  One CALL:
//       key=value,... with rows gates phase fields(hex) products rpb nx ny (a uniform grid of unit cells from 0) nz (layers of 500 m)
//       tK=N (field K has N thresholds 1, 2 ...) wK=N (field K has a weight table of N breakpoints 1, 2 ... N with the values 0.5,
//       1.0 ...) wvK / wfK (index:value -- one breakpoint or value of field K's table replaced; 'null': a NULL pointer) sum(0: NULL
//       sum of every field) skip(0: NULL sum_skipped)
// prints one line per call:
//   refused <reason> | gates G open o
//   ok blocks B cells C block_cells K zero Z state S total T open o gates G | field K max O count O top O sum O skip O weight N
// (gates: the gates folded into one block of the pass as the pass stands after the call)
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
    static double sum_sink[1];
    static uint32_t skip_sink[1];
    static const double ray[1] = {0.0};
    for (int i = 1; i < argc; ++i) {
        const std::string call = argv[i];
        std::map<std::string, std::string> kv;
        for (size_t p = 0; p < call.size();) {
            size_t q = call.find(',', p);
            if (q == std::string::npos) q = call.size();
            const std::string item = call.substr(p, q - p);
            const size_t eq = item.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad item '%s'\n", item.c_str()); return 2; }
            kv[item.substr(0, eq)] = item.substr(eq + 1);
            p = q + 1;
        }
        const auto num = [&](const std::string &k, long dflt) { return kv.count(k) ? strtol(kv[k].c_str(), nullptr, 0) : dflt; };
        CompCall c;
        c.n_rows = num("rows", 1); c.n_gates = (int)num("gates", 1);
        cpol_composite_sums w;
        memset(&w, 0, sizeof w);
        cpol_composite &s = w.c;
        s.fields = (uint32_t)num("fields", 1); s.phase = (int32_t)num("phase", 3); s.products = (uint32_t)num("products", 257);
        s.rays_per_block = (int32_t)num("rpb", 0);
        s.n_x = (int32_t)num("nx", 1); s.n_y = (int32_t)num("ny", 1);
        std::vector<double> ex, ey, ez;
        for (int j = 0; j <= s.n_x; ++j) ex.push_back((double)j);
        for (int j = 0; j <= s.n_y; ++j) ey.push_back((double)j);
        s.edges_x = ex.data(); s.edges_y = ey.data();
        s.ray_sin = ray; s.ray_cos = ray;
        s.n_z = (int32_t)num("nz", 0);
        for (int j = 0; j <= s.n_z && j <= 4096; ++j) ez.push_back(500.0 * j);
        if (s.n_z != 0) s.edges_z = ez.data();
        s.count = count_sink;
        std::vector<float> wv[COMP_FIELDS];
        std::vector<double> wf[COMP_FIELDS];
        for (int k = 0; k < COMP_FIELDS; ++k) {
            s.values[k] = value_sink;
            s.n_thresholds[k] = (int32_t)num("t" + std::to_string(k), 0);
            for (int j = 0; j < s.n_thresholds[k] && j < COMP_MAX_THR; ++j) s.thresholds[k][j] = 1.0 + j;
            const long n = num("w" + std::to_string(k), 0);
            w.n_weight[k] = (int32_t)n;
            for (long j = 0; j < n && j < 4096; ++j) { wv[k].push_back(1.0f + (float)j); wf[k].push_back(0.5 * (double)(j + 1)); }
            if (n) { w.weight_v[k] = wv[k].data(); w.weight_f[k] = wf[k].data(); }
            for (const char *which : {"wv", "wf"}) {
                const std::string key = which + std::to_string(k);
                if (!kv.count(key)) continue;
                if (kv[key] == "null") { if (which[1] == 'v') w.weight_v[k] = nullptr; else w.weight_f[k] = nullptr; continue; }
                const size_t colon = kv[key].find(':');
                if (colon == std::string::npos) { fprintf(stderr, "bad %s\n", key.c_str()); return 2; }
                const long at = strtol(kv[key].substr(0, colon).c_str(), nullptr, 0);
                const double v = strtod(kv[key].substr(colon + 1).c_str(), nullptr);
                if (at < 0 || at >= (long)wv[k].size()) { fprintf(stderr, "bad index in %s\n", key.c_str()); return 2; }
                if (which[1] == 'v') wv[k][(size_t)at] = (float)v; else wf[k][(size_t)at] = v;
            }
            if (num("sum", 1)) w.sum[k] = sum_sink;
            if (num("skip", 1)) w.sum_skipped[k] = skip_sink;
        }
        CompPlan pl;
        // (without the bit nothing behind `c` may be read: the sanitizer sees a narrow struct of its own then)
        const char *why;
        if (s.products & CPOL_COMP_SUM) why = comp_check(&s, c, pass, &pl);
        else {
            cpol_composite *const narrow = new cpol_composite(s);
            why = comp_check(narrow, c, pass, &pl);
            if (!why) comp_advance(narrow, pl, &pass);
            delete narrow;
        }
        if (why) { printf("refused %s | gates %llu open %d\n", why, pass.sum_gates, (int)pass.open); continue; }
        if (s.products & CPOL_COMP_SUM) comp_advance(&s, pl, &pass);
        printf("ok blocks %ld cells %ld block_cells %ld zero %ld state %ld total %ld open %d gates %llu", pl.n_blocks, pl.cells, pl.block_cells,
               pl.zero_bytes, pl.state_bytes, pl.total_bytes, (int)pass.open, pass.sum_gates);
        for (int j = 0; j < pl.n_fields; ++j) {
            const int k = pl.field[j];
            printf(" | field %d max %ld count %ld top %ld sum %ld skip %ld weight %zu", k, pl.off_max[k], pl.off_count[k], pl.off_top[k], pl.off_sum[k],
                   pl.off_skip[k], pl.wv[k].size());
        }
        printf("\n");
    }
    return 0;
}
