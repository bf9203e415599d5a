// Host check of the validation of the neighbourhood ensemble probabilities (cpol_fraction_probabilities: frac_prob_check and
// frac_prob_overflows in cosmo_pol_amd/csrc/cpol_frac.h); tests/test_neighbourhood_prob_cpu.py drives it.
//   frac_prob_check CALL ...     independent calls.  One CALL: key=value,... -- nx ny blocks (the maps), r (the largest radius; the
//       radii are 0 and r, or r alone when r is 0), nthr (thresholds, 1 by default), prob (0: NULL pointer), flag (0: n_radii without
//       CPOL_FRAC_ENSEMBLE), nrad (n_radii as given, flag bits and all), psums rel (0: NULL),
//       msum many (1: the map is asked for)
// prints one line per call:
//   overflow V | refused <reason>
//   overflow V | ok on O grid G entries E psums A rel B msum C many D
// V: what frac_prob_overflows answers for the numbers alone (the condition itself, whatever else refuses the call).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "cpol_frac.h"

int main(int argc, char **argv)
{
    static uint64_t sums_sink[1], totals_sink[1], psums_sink[1], rel_sink[1];
    static uint32_t msum_sink[1], many_sink[1];
    static float obs_sink[1];
    for (int i = 1; i < argc; ++i) {
        const std::string call = argv[i];
        std::map<std::string, std::string> kv;
        for (size_t p = 0; p < call.size();) {
            size_t q = call.find(',', p);
            if (q == std::string::npos) q = call.size();
            const std::string item = call.substr(p, q - p);
            p = q + 1;
            if (item.empty()) continue;
            const size_t eq = item.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad item '%s'\n", item.c_str()); return 2; }
            kv[item.substr(0, eq)] = item.substr(eq + 1);
        }
        const auto num = [&](const char *k, long dflt) { return kv.count(k) ? strtol(kv[k].c_str(), nullptr, 0) : dflt; };
        const int nx = (int)num("nx", 3), ny = (int)num("ny", 2), r = (int)num("r", 1);
        const long blocks = num("blocks", 2);
        cpol_fraction_probabilities q;
        memset(&q, 0, sizeof q);
        if (num("psums", 1)) q.prob_sums = psums_sink;
        if (num("rel", 1)) q.reliability = rel_sink;
        if (num("msum", 0)) q.member_sum = msum_sink;
        if (num("many", 0)) q.member_any = many_sink;
        // the cpol_fractions as the first member of a cpol_fractions_ensemble; flag=0: without CPOL_FRAC_ENSEMBLE in n_radii
        cpol_fractions_ensemble fe;
        memset(&fe, 0, sizeof fe);
        cpol_fractions &f = fe.f;
        f.n_thresholds = (int32_t)num("nthr", 1);
        for (int j = 0; j < f.n_thresholds && j < FRAC_MAX_THR; ++j) f.thresholds[j] = 1.0 + j;
        if (r > 0) { f.n_radii = 2; f.radii[0] = 0; f.radii[1] = r; }
        else { f.n_radii = 1; f.radii[0] = 0; }
        f.observed = obs_sink; f.sums = sums_sink; f.totals = totals_sink;
        if (num("prob", 1)) fe.probabilities = &q;
        if (num("flag", 1)) f.n_radii |= CPOL_FRAC_ENSEMBLE;
        if (kv.count("nrad")) f.n_radii = (int32_t)num("nrad", 0);
        printf("overflow %d | ", frac_prob_overflows(nx, ny, blocks, r) ? 1 : 0);
        FracPlan pl;
        const char *why = frac_check_maps(&f, nx, ny, blocks, &pl);
        if (why) { printf("refused %s\n", why); continue; }
        const FracProbPlan &pp = pl.prob;
        printf("ok on %d grid %ld entries %d psums %zu rel %zu msum %zu many %zu\n", pp.on ? 1 : 0, pp.grid, pp.table_entries,
               pp.prob_sums_bytes, pp.reliability_bytes, pp.member_sum_bytes, pp.member_any_bytes);
    }
    return 0;
}
