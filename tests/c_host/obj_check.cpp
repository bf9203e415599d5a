// Host check of the object cells' validation and labelling pieces (cosmo_pol_amd/csrc/cpol_obj.h); tests/test_objects_cpu.py
// drives it.
//   obj_check check CALL ...   independent calls.  One CALL: key=value,... -- of the maps: nx ny blocks nthr; of the cpol_objects:
//       obj(0: NULL struct) conn area max n(0: NULL n_objects) table(0: NULL, 4: misaligned by 4 bytes) labels(1: given)
//     prints one line per call:
//       refused <reason>
//       off
//       ok maps M cells C scratch S rows R cellgroups G decode D n N table T labels L
//   obj_check label FILE ...   FILE: int32 {n_y, n_x, connectivity, min_area}, uint8 flags [n_y][n_x], int32 labels [n_y][n_x] (the
//       rule's).  The run, union and find code of cpol_obj.h driven single-threaded exactly as the kernels cut the work -- a row in
//       chunks of 64 cells with the ballot of the flags, obj_merge_cell per cell, obj_find per cell, areas at the roots, the kept
//       roots numbered in raster order -- and compared with the labels of the file.
//     prints one line per file:
//       ok objects N runs R roots O      (O: the objects before the filter; R - O unions joined two objects)
//       mismatch cell I got G want W
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    alignas(8) static uint32_t n_sink[1], table_sink[4];
    static int32_t labels_sink[1];
    cpol_fractions f;
    memset(&f, 0, sizeof f);
    f.n_thresholds = (int32_t)num("nthr", 1); f.n_radii = 1;
    f.observed = obs_sink; f.sums = sums_sink; f.totals = totals_sink;
    FracPlan fp;
    const char *why = frac_check_maps(&f, (int)num("nx", 3), (int)num("ny", 2), num("blocks", 1), &fp);
    if (why) { printf("fractions refused %s\n", why); return 0; }
    cpol_objects o;
    memset(&o, 0, sizeof o);
    o.connectivity = (int32_t)num("conn", 4); o.min_area = (int32_t)num("area", 1); o.max_objects = (int32_t)num("max", 16);
    if (num("n", 1)) o.n_objects = n_sink;
    const long tab = num("table", 1);
    if (tab) o.table = tab == 4 ? table_sink + 1 : table_sink;
    if (num("labels", 0)) o.labels = labels_sink;
    ObjPlan pl;
    why = obj_check(num("obj", 1) ? &o : nullptr, fp, &pl);
    if (why) { printf("refused %s\n", why); return 0; }
    if (!pl.on) { printf("off\n"); return 0; }
    printf("ok maps %ld cells %ld scratch %ld rows %ld cellgroups %ld decode %ld n %zu table %zu labels %zu\n", pl.n_maps, pl.cells,
           pl.scratch_bytes, pl.grid_rows, pl.grid_cells, pl.grid_decode, pl.n_bytes, pl.table_bytes, pl.labels_bytes);
    return 0;
}

static int label(const char *path)
{
    FILE *fh = fopen(path, "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    int32_t head[4];
    if (fread(head, sizeof head, 1, fh) != 1) { fclose(fh); fprintf(stderr, "short file %s\n", path); return 2; }
    const int n_y = head[0], n_x = head[1], conn = head[2], min_area = head[3];
    if (n_y < 1 || n_x < 1 || n_y > FRAC_MAX_SIDE || n_x > FRAC_MAX_SIDE) { fclose(fh); fprintf(stderr, "bad grid\n"); return 2; }
    const size_t cells = (size_t)n_y * n_x;
    std::vector<uint8_t> flag(cells);
    std::vector<int32_t> want(cells);
    const bool read = fread(flag.data(), 1, cells, fh) == cells && fread(want.data(), 4, cells, fh) == cells;
    fclose(fh);
    if (!read) { fprintf(stderr, "short file %s\n", path); return 2; }
    std::vector<unsigned> L(cells), aux(cells, 0u);
    long runs = 0;
    // k_obj_runs: a row in chunks of 64 cells, the ballot of the flags, the carry across the chunks
    for (int y = 0; y < n_y; ++y) {
        int carry = -1;
        for (int x0 = 0; x0 < n_x; x0 += 64) {
            unsigned long long m = 0ull;
            for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane)
                if (flag[(size_t)y * n_x + x0 + lane]) m |= 1ull << lane;
            for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane) {
                const bool set = (m >> lane) & 1ull;
                unsigned first = OBJ_NONE;
                if (set) first = (unsigned)(y * n_x + (obj_run_open(m, lane) && carry >= 0 ? carry : x0 + obj_run_first(m, lane)));
                L[(size_t)y * n_x + x0 + lane] = first;
                if (set && first == (unsigned)(y * n_x + x0 + lane)) ++runs;
            }
            carry = obj_carry(m, x0, carry);
        }
    }
    // k_obj_merge
    for (int y = 1; y < n_y; ++y)
        for (int x = 0; x < n_x; ++x) obj_merge_cell(L.data(), n_x, y, x, conn);
    // k_obj_flatten
    for (size_t i = 0; i < cells; ++i)
        if (L[i] != OBJ_NONE) L[i] = obj_find(L.data(), (unsigned)i);
    // k_obj_area: one addition per run segment of a chunk
    for (int y = 0; y < n_y; ++y)
        for (int x0 = 0; x0 < n_x; x0 += 64) {
            unsigned long long m = 0ull;
            for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane)
                if (L[(size_t)y * n_x + x0 + lane] != OBJ_NONE) m |= 1ull << lane;
            for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane)
                if (((m >> lane) & 1ull) && (lane == 0 || !((m >> (lane - 1)) & 1ull)))
                    aux[L[(size_t)y * n_x + x0 + lane]] += (unsigned)obj_run_len(m, lane);
        }
    // k_obj_count / k_obj_number: the kept roots in raster order
    unsigned n = 0u;
    long roots = 0;
    for (size_t i = 0; i < cells; ++i)
        if (L[i] == (unsigned)i) { ++roots; aux[i] = aux[i] >= (unsigned)min_area ? ++n : 0u; }
    for (size_t i = 0; i < cells; ++i) {
        const int32_t got = L[i] == OBJ_NONE ? 0 : (int32_t)aux[L[i]];
        if (got != want[i]) { printf("mismatch cell %zu got %d want %d\n", i, got, want[i]); return 0; }
    }
    printf("ok objects %u runs %ld roots %ld\n", n, runs, roots);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2 || (strcmp(argv[1], "check") && strcmp(argv[1], "label"))) { fprintf(stderr, "usage: obj_check check CALL ... | label FILE ...\n"); return 2; }
    for (int i = 2; i < argc; ++i) {
        const int rc = argv[1][0] == 'c' ? check(argv[i]) : label(argv[i]);
        if (rc) return rc;
    }
    return 0;
}
