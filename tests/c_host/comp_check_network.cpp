// Host check of the NETWORK additions to the composite validation (cosmo_pol_amd/csrc/cpol_comp.h: the plane, the source, the
// source bytes and the scratch state); tests/test_composite_network_cpu.py drives it.  comp_check.cpp covers everything else.
//   comp_check_network CALL ...   the calls of one context in turn; the pass they open and close is kept between them.  One CALL:
//       key=value,... with rows gates space phase fields(hex) products rpb nx ny (a uniform grid of unit cells from 0) plane
//       source rays(0: NULL ray_sin / ray_cos) gx(0: NULL gate_x) gy(0: NULL gate_y) and tK=N (field K has N thresholds 1, 2 ...)
// prints one line per call:
//   refused <reason>
//   ok blocks B cells C zero Z state S total T scratch O plane P source N with_source W open o | field K planes P max O count O top
//   O low O src_max O src_low O
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
        c.spaceborne = num("space", 0) != 0;
        cpol_composite s;
        memset(&s, 0, sizeof s);
        s.fields = (uint32_t)num("fields", 1); s.phase = (int32_t)num("phase", 3); s.products = (uint32_t)num("products", 1);
        s.rays_per_block = (int32_t)num("rpb", 0);
        s.n_x = (int32_t)num("nx", 1); s.n_y = (int32_t)num("ny", 1);
        std::vector<double> ex, ey;
        for (int j = 0; j <= s.n_x; ++j) ex.push_back((double)j);
        for (int j = 0; j <= s.n_y; ++j) ey.push_back((double)j);
        s.edges_x = ex.data(); s.edges_y = ey.data();
        s.plane = (int32_t)num("plane", 0); s.source = (int32_t)num("source", 0);
        if (num("rays", 1)) { s.ray_sin = ray; s.ray_cos = ray; }
        if (num("gx", 1)) s.gate_x = gate;
        if (num("gy", 1)) s.gate_y = gate;
        s.count = count_sink;
        for (int k = 0; k < COMP_FIELDS; ++k) {
            s.values[k] = value_sink;
            s.n_thresholds[k] = (int32_t)num("t" + std::to_string(k), 0);
            for (int j = 0; j < s.n_thresholds[k] && j < COMP_MAX_THR; ++j) s.thresholds[k][j] = 1.0 + j;
        }
        CompPlan pl;
        const char *why = comp_check(&s, c, pass, &pl);
        if (why) { printf("refused %s\n", why); continue; }
        comp_advance(&s, pl, &pass);
        printf("ok blocks %ld cells %ld zero %ld state %ld total %ld scratch %ld plane %d source %d with_source %d open %d", pl.n_blocks, pl.cells,
               pl.zero_bytes, pl.state_bytes, pl.total_bytes, pl.off_scratch, pl.plane, pl.source, (int)pl.with_source, (int)pass.open);
        for (int j = 0; j < pl.n_fields; ++j) {
            const int k = pl.field[j];
            printf(" | field %d planes %d max %ld count %ld top %ld low %ld src_max %ld src_low %ld", k, pl.n_planes[k], pl.off_max[k],
                   pl.off_count[k], pl.off_top[k], pl.off_low[k], pl.off_src_max[k], pl.off_src_low[k]);
        }
        printf("\n");
    }
    return 0;
}
