// Host check of the exact sums of the object cells (cosmo_pol_amd/csrc/cpol_obj.h); tests/test_object_sums_cpu.py drives it.
//   obj_sums_check check CALL ...   independent calls.  One CALL: key=value,... -- of the maps: nx ny blocks nthr; of the
//       cpol_objects: max sums(0, 1 or any other number) vol(0: NULL, 4: misaligned by 4 bytes) skipped(0: NULL) field(0, 4)
//       cells(0: NULL) nw(n_weight) wv(0: NULL) wf(0: NULL) tab(ok | flat: two equal breakpoints | desc: values that decrease |
//       nan: a NaN value | inf: an infinite breakpoint)
//     prints one line per call:
//       refused <reason>
//       ok sums S scratch B acc_offset A acc_bytes C weight_offset W finish G volume V skipped K field F field_cells L
//   obj_sums_check sum FILE ...   FILE: int32 n, then uint32 bits [n] (float32 summands), int32 ix [n], int32 iy [n].  The split,
//       the accumulator row and the rounding of cpol_obj.h single-threaded, every addition into a bin checked for overflow.
//     prints one line per file:
//       ok VOLUME MOMENT_X MOMENT_Y skipped K      (the float64 bits in hexadecimal)
//       wrap bin B
//   obj_sums_check weight FILE ...  FILE: int32 n_tab, int32 n, float32 tv [n_tab], float64 tf [n_tab], float32 values [n]
//     prints one line per file: the float32 bits of obj_weight of every value in hexadecimal
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>
#include "cpol_obj.h"

static int check(const std::string &call)
{
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
    static float obs_sink[1];
    static uint64_t sums_sink[1], totals_sink[1];
    alignas(8) static uint32_t n_sink[1], table_sink[4], skipped_sink[1], cells_sink[2];
    alignas(8) static uint32_t volume_sink[4], field_sink[4];         // (uint32 storage: a pointer misaligned by 4 bytes is formed, never read)
    cpol_fractions f;
    memset(&f, 0, sizeof f);
    f.n_thresholds = (int32_t)num("nthr", 1); f.n_radii = 1;
    f.observed = obs_sink; f.sums = sums_sink; f.totals = totals_sink;
    FracPlan fp;
    const char *why = frac_check_maps(&f, (int)num("nx", 3), (int)num("ny", 2), num("blocks", 1), &fp);
    if (why) { printf("fractions refused %s\n", why); return 0; }
    cpol_objects o;
    memset(&o, 0, sizeof o);
    o.connectivity = 4; o.min_area = 1; o.max_objects = (int32_t)num("max", 16);
    o.n_objects = n_sink; o.table = table_sink;
    o.sums = (int32_t)num("sums", 1);
    const long vol = num("vol", 1), fld = num("field", 1);
    if (vol) o.volume = (double *)(void *)(vol == 4 ? volume_sink + 1 : volume_sink);
    if (fld) o.field = (double *)(void *)(fld == 4 ? field_sink + 1 : field_sink);
    if (num("skipped", 1)) o.skipped = skipped_sink;
    if (num("cells", 1)) o.field_cells = cells_sink;
    const long nw = num("nw", 0);
    std::vector<float> tv((size_t)(nw > 0 ? nw : 0));
    std::vector<double> tf(tv.size());
    for (size_t j = 0; j < tv.size(); ++j) { tv[j] = (float)(j + 1); tf[j] = 0.5 * (double)(j / 2); }      // (values that stay equal in pairs)
    const std::string tab = kv.count("tab") ? kv["tab"] : "ok";
    if (tv.size() >= 2) {
        if (tab == "flat") tv[1] = tv[0];
        if (tab == "desc") tf[tf.size() - 1] = -1.0;
        if (tab == "nan") tf[0] = std::numeric_limits<double>::quiet_NaN();
        if (tab == "inf") tv[tv.size() - 1] = std::numeric_limits<float>::infinity();
    }
    o.n_weight = (int32_t)nw;
    if (num("wv", 1)) o.weight_v = tv.data();
    if (num("wf", 1)) o.weight_f = tf.data();
    ObjPlan pl;
    why = obj_check(&o, fp, &pl);
    if (why) { printf("refused %s\n", why); return 0; }
    printf("ok sums %d scratch %ld acc_offset %ld acc_bytes %ld weight_offset %ld finish %ld volume %zu skipped %zu field %zu field_cells %zu\n",
           (int)pl.sums, pl.scratch_bytes, pl.acc_offset, pl.acc_bytes, pl.weight_offset, pl.grid_finish, pl.volume_bytes, pl.skipped_bytes,
           pl.field_bytes, pl.field_cells_bytes);
    return 0;
}

static bool read_all(const char *path, std::vector<unsigned char> *buf)
{
    FILE *fh = fopen(path, "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", path); return false; }
    unsigned char chunk[1 << 16];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, fh)) > 0) buf->insert(buf->end(), chunk, chunk + n);
    fclose(fh);
    return true;
}

static int sum(const char *path)
{
    std::vector<unsigned char> buf;
    if (!read_all(path, &buf)) return 2;
    int32_t n;
    if (buf.size() < 4) { fprintf(stderr, "short file %s\n", path); return 2; }
    memcpy(&n, buf.data(), 4);
    if (n < 0 || buf.size() != 4 + (size_t)n * 12) { fprintf(stderr, "bad file %s\n", path); return 2; }
    std::vector<uint32_t> bits((size_t)n);
    std::vector<int32_t> ix((size_t)n), iy((size_t)n);
    if (n) {
        memcpy(bits.data(), buf.data() + 4, (size_t)n * 4);
        memcpy(ix.data(), buf.data() + 4 + (size_t)n * 4, (size_t)n * 4);
        memcpy(iy.data(), buf.data() + 4 + (size_t)n * 8, (size_t)n * 4);
    }
    long long acc[OBJ_SUM_BINS] = {};
    unsigned skipped = 0u;
    for (int32_t i = 0; i < n; ++i) {
        int E; unsigned M;
        if (!obj_sum_split(bits[(size_t)i], &E, &M)) { ++skipped; continue; }
        if (ix[(size_t)i] < 0 || ix[(size_t)i] > 1023 || iy[(size_t)i] < 0 || iy[(size_t)i] > 1023) { fprintf(stderr, "bad index\n"); return 2; }
        const int b = E >> 3;
        const int at[3] = {b >> 1, OBJ_SUM_VOL_BINS + b, OBJ_SUM_VOL_BINS + OBJ_SUM_MOM_BINS + b};
        const long long c[3] = {obj_sum_term(bits[(size_t)i], M, 1u, E & 15), obj_sum_term(bits[(size_t)i], M, (unsigned)ix[(size_t)i], E & 7),
                                obj_sum_term(bits[(size_t)i], M, (unsigned)iy[(size_t)i], E & 7)};
        for (int k = 0; k < 3; ++k)
            if (__builtin_add_overflow(acc[at[k]], c[k], &acc[at[k]])) { printf("wrap bin %d\n", at[k]); return 0; }
    }
    unsigned long long u[OBJ_SUM_BINS];
    for (int k = 0; k < OBJ_SUM_BINS; ++k) u[k] = (unsigned long long)acc[k];
    printf("ok %016llx %016llx %016llx skipped %u\n", obj_sum_round(u, OBJ_SUM_VOL_BINS, 16), obj_sum_round(u + OBJ_SUM_VOL_BINS, OBJ_SUM_MOM_BINS, 8),
           obj_sum_round(u + OBJ_SUM_VOL_BINS + OBJ_SUM_MOM_BINS, OBJ_SUM_MOM_BINS, 8), skipped);
    return 0;
}

static int weight(const char *path)
{
    std::vector<unsigned char> buf;
    if (!read_all(path, &buf)) return 2;
    int32_t head[2];
    if (buf.size() < 8) { fprintf(stderr, "short file %s\n", path); return 2; }
    memcpy(head, buf.data(), 8);
    const int n_tab = head[0], n = head[1];
    if (n_tab < 2 || n_tab > COMP_MAX_TABLE || n < 0 || buf.size() != 8 + (size_t)n_tab * 12 + (size_t)n * 4) { fprintf(stderr, "bad file %s\n", path); return 2; }
    std::vector<float> tv((size_t)n_tab), v((size_t)n);
    std::vector<double> tf((size_t)n_tab);
    memcpy(tv.data(), buf.data() + 8, (size_t)n_tab * 4);
    memcpy(tf.data(), buf.data() + 8 + (size_t)n_tab * 4, (size_t)n_tab * 8);
    if (n) memcpy(v.data(), buf.data() + 8 + (size_t)n_tab * 12, (size_t)n * 4);
    int step0 = 1;
    while (2 * step0 <= n_tab) step0 *= 2;
    for (int i = 0; i < n; ++i) {
        const float w = obj_weight(tv.data(), tf.data(), n_tab, step0, v[(size_t)i]);
        uint32_t b;
        memcpy(&b, &w, 4);
        printf(i ? " %08x" : "%08x", b);
    }
    printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2 || (strcmp(argv[1], "check") && strcmp(argv[1], "sum") && strcmp(argv[1], "weight"))) {
        fprintf(stderr, "usage: obj_sums_check check CALL ... | sum FILE ... | weight FILE ...\n");
        return 2;
    }
    for (int i = 2; i < argc; ++i) {
        const int rc = argv[1][0] == 'c' ? check(argv[i]) : argv[1][0] == 's' ? sum(argv[i]) : weight(argv[i]);
        if (rc) return rc;
    }
    return 0;
}
