// Host check of the one-product rule (cosmo_pol_amd/csrc/cpol_products.h); tests/test_call_product_cpu.py drives it.
//   products_check ENTRY SET ...   ENTRY: sweep / members / timed / columns; one SET per call: the pointers of cpol_outputs that are
//                                  set, as a comma list of superob member_stats member_verify spectrum_moments histogram composite
//                                  fractions ("-": none)
// prints one line per SET, tab-separated:  PRODUCT WHEN TEXT   with WHEN one of  accepted / entry (refused by the entry point itself)
// / before (refused before any product's plan) / after (refused once the product's plan has passed)  and TEXT the refusal ("-": none)
#include <cstdio>
#include <cstring>
#include <string>
#include "cpol_products.h"

int main(int argc, char **argv)
{
    static const char *const entries[] = {"sweep", "members", "timed", "columns"};
    static const char *const products[] = {"none", "superob", "member_stats", "spectrum_moments", "histogram", "composite"};
    int entry = -1;
    for (int e = 0; e < 4 && argc > 1; ++e)
        if (!strcmp(argv[1], entries[e])) entry = e;
    if (entry < 0) { fprintf(stderr, "usage: products_check sweep|members|timed|columns SET ...\n"); return 2; }
    // (call_product looks at the pointers alone: each set one points at a zeroed struct of its type)
    static cpol_superob so; static cpol_member_stats ms; static cpol_member_verify mv; static cpol_spectrum_moments sm;
    static cpol_histogram hg; static cpol_composite cp; static cpol_fractions fr;
    for (int i = 2; i < argc; ++i) {
        cpol_outputs o;
        memset(&o, 0, sizeof o);
        const std::string set = std::string(",") + argv[i] + ",";
        const auto has = [&](const char *name) { return set.find(std::string(",") + name + ",") != std::string::npos; };
        if (has("superob")) o.superob = &so;
        if (has("member_stats")) o.member_stats = &ms;
        if (has("member_verify")) o.member_verify = &mv;
        if (has("spectrum_moments")) o.spectrum_moments = &sm;
        if (has("histogram")) o.histogram = &hg;
        if (has("composite")) o.composite = &cp;
        if (has("fractions")) o.fractions = &fr;
        const CallProduct r = call_product(entry, o);
        if (r.refuse && r.refuse_after_plan) { fprintf(stderr, "two refusals for '%s'\n", argv[i]); return 1; }
        const char *const when = r.refuse ? (r.at_entry ? "entry" : "before") : r.refuse_after_plan ? "after" : "accepted";
        const char *const text = r.refuse ? r.refuse : r.refuse_after_plan ? r.refuse_after_plan : "-";
        printf("%s\t%s\t%s\n", products[r.product], when, text);
    }
    return 0;
}
