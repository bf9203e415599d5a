// Host check of the HEIGHT LAYERS and the COLUMN in the composite validation (cosmo_pol_amd/csrc/cpol_comp.h: the layer edges and
// their rounding, the tables, gaps, the state sizes with layers, the pass); tests/test_composite_layers_cpu.py drives it.
// comp_check.cpp and comp_check_network.cpp cover everything else.
//   comp_check_layers CALL ...   the calls of one context in turn; the pass they open and close is kept between them.  One CALL:
//       key=value,... with rows gates phase fields(hex) products rpb nx ny (a uniform grid of unit cells from 0) plane source slab
//       nz gaps ez (n_z + 1 edges separated by ':'; default 0, 500, 1000 ...; 'null': a NULL pointer) tabK=N (field K has a table of
//       N breakpoints 1, 2 ... N with the values 0.5, 1.0 ...) tvK / tfK (index:value -- one breakpoint or value of field K's table
//       replaced; 'null': a NULL pointer) col(0: NULL column of every field) lay(0: NULL column_layers) fr(1: frac_check of a
//       cpol_fractions beside the composite) and tK=N (field K has N thresholds 1, 2 ...)
// prints one line per call:
//   refused <reason>
//   ok blocks B cells C block_cells K nz Z gaps G column W zero Z state S total T open o ez0 E ezn E | field K planes P max O count O
//   table N
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "cpol_frac.h"

int main(int argc, char **argv)
{
    CompPass pass;
    static uint64_t count_sink[1];
    static float value_sink[1];
    static double column_sink[1];
    static uint8_t layers_sink[1];
    static const double ray[1] = {0.0}, gate[1] = {0.0};
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
        cpol_composite s;
        memset(&s, 0, sizeof s);
        s.fields = (uint32_t)num("fields", 1); s.phase = (int32_t)num("phase", 3); s.products = (uint32_t)num("products", 1);
        s.rays_per_block = (int32_t)num("rpb", 0);
        s.n_x = (int32_t)num("nx", 1); s.n_y = (int32_t)num("ny", 1);
        std::vector<double> ex, ey, ez;
        for (int j = 0; j <= s.n_x; ++j) ex.push_back((double)j);
        for (int j = 0; j <= s.n_y; ++j) ey.push_back((double)j);
        s.edges_x = ex.data(); s.edges_y = ey.data();
        s.plane = (int32_t)num("plane", 0); s.source = (int32_t)num("source", 0);
        s.ray_sin = ray; s.ray_cos = ray; s.gate_x = gate; s.gate_y = gate;
        if (num("slab", 0)) { s.use_slab = 1; s.h_lo = 0.0; s.h_hi = 1000.0; }
        s.n_z = (int32_t)num("nz", 0); s.gaps = (int32_t)num("gaps", 0);
        if (kv.count("ez") && kv["ez"] != "null") {
            const std::string &e = kv["ez"];
            for (size_t p = 0; p < e.size();) {
                size_t q = e.find(':', p);
                if (q == std::string::npos) q = e.size();
                ez.push_back(strtod(e.substr(p, q - p).c_str(), nullptr));
                p = q + 1;
            }
            if ((long)ez.size() < (long)s.n_z + 1) { fprintf(stderr, "ez: %zu edges for nz=%d\n", ez.size(), s.n_z); return 2; }
        } else
            for (int j = 0; j <= s.n_z && j <= 4096; ++j) ez.push_back(500.0 * j);
        if (!(kv.count("ez") && kv["ez"] == "null") && s.n_z != 0) s.edges_z = ez.data();
        s.count = count_sink;
        std::vector<float> tv[COMP_FIELDS];
        std::vector<double> tf[COMP_FIELDS];
        for (int k = 0; k < COMP_FIELDS; ++k) {
            s.values[k] = value_sink;
            s.n_thresholds[k] = (int32_t)num("t" + std::to_string(k), 0);
            for (int j = 0; j < s.n_thresholds[k] && j < COMP_MAX_THR; ++j) s.thresholds[k][j] = 1.0 + j;
            const long n = num("tab" + std::to_string(k), 0);
            s.n_table[k] = (int32_t)n;
            for (long j = 0; j < n && j < 4096; ++j) { tv[k].push_back(1.0f + (float)j); tf[k].push_back(0.5 * (double)(j + 1)); }
            if (n) { s.table_v[k] = tv[k].data(); s.table_f[k] = tf[k].data(); }
            for (const char *which : {"tv", "tf"}) {
                const std::string key = which + std::to_string(k);
                if (!kv.count(key)) continue;
                if (kv[key] == "null") { if (which[1] == 'v') s.table_v[k] = nullptr; else s.table_f[k] = nullptr; continue; }
                const size_t colon = kv[key].find(':');
                if (colon == std::string::npos) { fprintf(stderr, "bad %s\n", key.c_str()); return 2; }
                const long at = strtol(kv[key].substr(0, colon).c_str(), nullptr, 0);
                const double v = strtod(kv[key].substr(colon + 1).c_str(), nullptr);
                if (at < 0 || at >= (long)tv[k].size()) { fprintf(stderr, "bad index in %s\n", key.c_str()); return 2; }
                if (which[1] == 'v') tv[k][(size_t)at] = (float)v; else tf[k][(size_t)at] = v;
            }
            if (num("col", 1)) s.column[k] = column_sink;
            if (num("lay", 1)) s.column_layers[k] = layers_sink;
        }
        CompPlan pl;
        const char *why = comp_check(&s, c, pass, &pl);
        if (why) { printf("refused %s\n", why); continue; }
        if (num("fr", 0)) {
            static uint64_t sums[64];
            static const float obs[1] = {0.f};
            cpol_fractions f;
            memset(&f, 0, sizeof f);
            f.n_thresholds = 1; f.n_radii = 1; f.thresholds[0] = 1.0; f.observed = obs; f.sums = sums; f.totals = sums;
            FracPlan fp;
            const char *why_f = frac_check(&f, &s, &pl, &fp);
            if (why_f) { printf("refused fractions: %s\n", why_f); continue; }
        }
        comp_advance(&s, pl, &pass);
        printf("ok blocks %ld cells %ld block_cells %ld nz %d gaps %d column %d zero %ld state %ld total %ld open %d ez0 %a ezn %a", pl.n_blocks,
               pl.cells, pl.block_cells, pl.n_z, pl.gaps, (int)pl.column, pl.zero_bytes, pl.state_bytes, pl.total_bytes, (int)pass.open,
               pl.ez.empty() ? 0.0 : (double)pl.ez.front(), pl.ez.empty() ? 0.0 : (double)pl.ez.back());
        for (int j = 0; j < pl.n_fields; ++j) {
            const int k = pl.field[j];
            printf(" | field %d planes %d max %ld count %ld table %zu", k, pl.n_planes[k], pl.off_max[k], pl.off_count[k], pl.tv[k].size());
        }
        printf("\n");
    }
    return 0;
}
