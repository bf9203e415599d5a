// Host check of the match's validation and per-cell pieces (cosmo_pol_amd/csrc/cpol_obj.h); tests/test_object_match_cpu.py drives it.
//   obj_match_check check CALL ...   independent calls.  One CALL: key=value,... -- of the maps: nx ny blocks nthr; of the cpol_objects:
//       conn area max labels sums(1: the exact sums on) weight(breakpoints of a weight table); of the match: pieces (pad_; 0: off, the
//       struct is then a bare cpol_objects with nothing behind it) np pc cov (0: NULL n_pieces, pieces, covered)
//     prints one line per call:
//       refused <reason>
//       ok scratch S match 0
//       ok scratch S match 1 maxpieces P piecemaps M offset O piecebytes B rows R cellgroups G decode D n N pieces T covered C
//   obj_match_check match FILE ...   FILE: int32 {n_y, n_x, connectivity, min_area, max_pieces, max_objects}, uint8 flags [n_y][n_x] of
//       the forecast map and of the observed map, then the rule's: int32 labels [n_y][n_x] of both, uint32 n_pieces, uint32 pieces
//       [max_pieces][10], uint32 covered [2][max_objects].  Both maps are labelled with the run, union and find code as the object
//       kernels cut the work (L flattened, aux[root] = the kept number or 0), then the match single-threaded as its kernels cut it:
//       per chunk of 64 cells obj_match_flag, the ballot, the run functions and obj_match_cover; merge, flatten, area and numbering
//       on the piece L; sums, box and the two numbers per run segment and root.
//     prints one line per file:
//       ok pieces N runs R            (R: the runs of the overlap map; R - N unions joined two pieces)
//       mismatch <what> at I got G want W
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
    alignas(8) static uint32_t n_sink[1], table_sink[4], u_sink[2];
    alignas(8) static double d_sink[1];
    static int32_t labels_sink[1];
    cpol_fractions f;
    memset(&f, 0, sizeof f);
    f.n_thresholds = (int32_t)num("nthr", 1); f.n_radii = 1;
    f.observed = obs_sink; f.sums = sums_sink; f.totals = totals_sink;
    FracPlan fp;
    const char *why = frac_check_maps(&f, (int)num("nx", 3), (int)num("ny", 2), num("blocks", 1), &fp);
    if (why) { printf("fractions refused %s\n", why); return 0; }
    // with pieces=0 the library must not read behind the cpol_objects: it gets a heap block of exactly sizeof(cpol_objects), so that
    // the address sanitizer sees any read beyond it
    const long pieces = num("pieces", 0);
    const bool bare = pieces == 0;
    std::vector<char> heap(bare ? sizeof(cpol_objects) : sizeof(cpol_objects_match), 0);
    cpol_objects *const o = (cpol_objects *)heap.data();
    o->connectivity = (int32_t)num("conn", 4); o->min_area = (int32_t)num("area", 1); o->max_objects = (int32_t)num("max", 16);
    o->n_objects = n_sink; o->table = table_sink;
    if (num("labels", 0)) o->labels = labels_sink;
    std::vector<float> wv;
    std::vector<double> wf;
    if (num("sums", 0)) {
        o->sums = 1; o->volume = d_sink; o->skipped = u_sink; o->field = d_sink; o->field_cells = u_sink;
        const long nw = num("weight", 0);
        for (long j = 0; j < nw; ++j) { wv.push_back((float)j); wf.push_back((double)j); }
        if (nw) { o->n_weight = (int32_t)nw; o->weight_v = wv.data(); o->weight_f = wf.data(); }
    }
    o->pad_ = (int32_t)pieces;
    if (!bare) {
        cpol_objects_match *const mo = (cpol_objects_match *)heap.data();
        if (num("np", 1)) mo->n_pieces = n_sink;
        if (num("pc", 1)) mo->pieces = table_sink;
        if (num("cov", 1)) mo->covered = u_sink;
    }
    ObjPlan pl;
    why = obj_check(o, fp, &pl);
    if (why) { printf("refused %s\n", why); return 0; }
    if (!pl.match) { printf("ok scratch %ld match 0\n", pl.scratch_bytes); return 0; }
    printf("ok scratch %ld match 1 maxpieces %d piecemaps %ld offset %ld piecebytes %ld rows %ld cellgroups %ld decode %ld n %zu pieces %zu covered %zu\n",
           pl.scratch_bytes, pl.max_pieces, pl.piece_maps, pl.piece_offset, pl.piece_bytes, pl.grid_piece_rows, pl.grid_piece_cells,
           pl.grid_piece_decode, pl.n_pieces_bytes, pl.pieces_bytes, pl.covered_bytes);
    return 0;
}

// the ballot of a chunk: bit l = flag(x0 + l)
template <class Flag>
static unsigned long long ballot(int n_x, int x0, Flag flag)
{
    unsigned long long m = 0ull;
    for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane)
        if (flag(x0 + lane)) m |= 1ull << lane;
    return m;
}

// k_obj_runs / k_match_runs: L = the first cell of the cell's row run; returns the runs.  begin(y, x0, lane, m): what the lane at which
// a run segment begins in a chunk does besides
template <class Flag, class Begin>
static long runs_of(int n_y, int n_x, std::vector<unsigned> &L, Flag flag, Begin begin)
{
    long runs = 0;
    for (int y = 0; y < n_y; ++y) {
        int carry = -1;
        for (int x0 = 0; x0 < n_x; x0 += 64) {
            const unsigned long long m = ballot(n_x, x0, [&](int x) { return flag(y, x); });
            for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane) {
                const bool set = (m >> lane) & 1ull;
                unsigned first = OBJ_NONE;
                if (set) first = (unsigned)(y * n_x + (obj_run_open(m, lane) && carry >= 0 ? carry : x0 + obj_run_first(m, lane)));
                L[(size_t)y * n_x + x0 + lane] = first;
                if (set && first == (unsigned)(y * n_x + x0 + lane)) ++runs;
                if (set && (lane == 0 || !((m >> (lane - 1)) & 1ull))) begin(y, x0, lane, m);
            }
            carry = obj_carry(m, x0, carry);
        }
    }
    return runs;
}

// k_obj_merge ... k_obj_number on the L that runs_of left: L flattened, aux[root] = the kept number or 0; returns the kept count
static unsigned number_of(int n_y, int n_x, int conn, int min_area, std::vector<unsigned> &L, std::vector<unsigned> &aux)
{
    const size_t cells = (size_t)n_y * n_x;
    for (int y = 1; y < n_y; ++y)
        for (int x = 0; x < n_x; ++x) obj_merge_cell(L.data(), n_x, y, x, conn);
    for (size_t i = 0; i < cells; ++i) {
        aux[i] = 0u;
        if (L[i] != OBJ_NONE) L[i] = obj_find(L.data(), (unsigned)i);
    }
    for (int y = 0; y < n_y; ++y)
        for (int x0 = 0; x0 < n_x; x0 += 64) {
            const unsigned long long m = ballot(n_x, x0, [&](int x) { return L[(size_t)y * n_x + x] != OBJ_NONE; });
            for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane)
                if (((m >> lane) & 1ull) && (lane == 0 || !((m >> (lane - 1)) & 1ull)))
                    aux[L[(size_t)y * n_x + x0 + lane]] += (unsigned)obj_run_len(m, lane);
        }
    unsigned n = 0u;
    for (size_t i = 0; i < cells; ++i)
        if (L[i] == (unsigned)i) aux[i] = aux[i] >= (unsigned)min_area ? ++n : 0u;
    return n;
}

static int match(const char *path)
{
    FILE *fh = fopen(path, "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    int32_t head[6];
    if (fread(head, sizeof head, 1, fh) != 1) { fclose(fh); fprintf(stderr, "short file %s\n", path); return 2; }
    const int n_y = head[0], n_x = head[1], conn = head[2], min_area = head[3], max_pieces = head[4], max_objects = head[5];
    if (n_y < 1 || n_x < 1 || n_y > FRAC_MAX_SIDE || n_x > FRAC_MAX_SIDE || max_pieces < 1 || max_pieces > OBJ_MAX_OBJECTS ||
        max_objects < 1 || max_objects > OBJ_MAX_OBJECTS) { fclose(fh); fprintf(stderr, "bad head\n"); return 2; }
    const size_t cells = (size_t)n_y * n_x;
    std::vector<uint8_t> flag_f(cells), flag_o(cells);
    std::vector<int32_t> want_f(cells), want_o(cells);
    uint32_t want_n = 0u;
    std::vector<uint32_t> want_pieces((size_t)max_pieces * OBJ_WORDS), want_cov((size_t)2 * max_objects);
    const bool read = fread(flag_f.data(), 1, cells, fh) == cells && fread(flag_o.data(), 1, cells, fh) == cells &&
                      fread(want_f.data(), 4, cells, fh) == cells && fread(want_o.data(), 4, cells, fh) == cells &&
                      fread(&want_n, 4, 1, fh) == 1 && fread(want_pieces.data(), 4, want_pieces.size(), fh) == want_pieces.size() &&
                      fread(want_cov.data(), 4, want_cov.size(), fh) == want_cov.size();
    fclose(fh);
    if (!read) { fprintf(stderr, "short file %s\n", path); return 2; }
    // the object phase of both maps
    std::vector<unsigned> Lf(cells), auxf(cells), Lo(cells), auxo(cells);
    const auto nothing = [](int, int, int, unsigned long long) {};
    runs_of(n_y, n_x, Lf, [&](int y, int x) { return flag_f[(size_t)y * n_x + x] != 0; }, nothing);
    runs_of(n_y, n_x, Lo, [&](int y, int x) { return flag_o[(size_t)y * n_x + x] != 0; }, nothing);
    number_of(n_y, n_x, conn, min_area, Lf, auxf);
    number_of(n_y, n_x, conn, min_area, Lo, auxo);
    for (size_t i = 0; i < cells; ++i) {
        const int32_t gf = (int32_t)obj_number_of(Lf.data(), auxf.data(), (unsigned)i), go = (int32_t)obj_number_of(Lo.data(), auxo.data(), (unsigned)i);
        if (gf != want_f[i]) { printf("mismatch forecast label at %zu got %d want %d\n", i, gf, want_f[i]); return 0; }
        if (go != want_o[i]) { printf("mismatch observed label at %zu got %d want %d\n", i, go, want_o[i]); return 0; }
    }
    // k_match_runs
    std::vector<unsigned> L(cells), aux(cells), covered((size_t)2 * max_objects, 0u);
    unsigned nf = 0u, no = 0u;
    const long runs = runs_of(n_y, n_x, L,
        [&](int y, int x) { return obj_match_flag(Lf.data(), auxf.data(), Lo.data(), auxo.data(), (unsigned)(y * n_x + x), &nf, &no); },
        [&](int y, int x0, int lane, unsigned long long m) {
            unsigned f, o;
            obj_match_flag(Lf.data(), auxf.data(), Lo.data(), auxo.data(), (unsigned)(y * n_x + x0 + lane), &f, &o);
            obj_match_cover(covered.data(), max_objects, f, o, (unsigned)obj_run_len(m, lane));
        });
    // the objects' kernels on the piece arrays: min_area 1
    const unsigned n = number_of(n_y, n_x, conn, 1, L, aux);
    // k_obj_number's rows, k_match_attr, k_match_decode
    std::vector<uint32_t> pieces((size_t)max_pieces * OBJ_WORDS, 0u);
    std::vector<unsigned> area(cells, 0u);
    for (size_t i = 0; i < cells; ++i)
        if (L[i] != OBJ_NONE) ++area[L[i]];
    for (int y = 0; y < n_y; ++y)
        for (int x0 = 0; x0 < n_x; x0 += 64) {
            const unsigned long long m = ballot(n_x, x0, [&](int x) { return L[(size_t)y * n_x + x] != OBJ_NONE; });
            for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane) {
                if (!((m >> lane) & 1ull)) continue;
                const unsigned cell = (unsigned)(y * n_x + x0 + lane), root = L[cell], number = aux[root];
                if (number == 0u || number > (unsigned)max_pieces) continue;
                uint32_t *const row = pieces.data() + (size_t)(number - 1u) * OBJ_WORDS;
                if (root == cell) {
                    row[OBJ_FIRST] = cell; row[OBJ_AREA] = area[root];
                    row[OBJ_PEAK_CELL] = obj_number_of(Lf.data(), auxf.data(), cell);
                    row[OBJ_PEAK_BITS] = obj_number_of(Lo.data(), auxo.data(), cell);
                }
                if (lane != 0 && ((m >> (lane - 1)) & 1ull)) continue;
                const unsigned len = (unsigned)obj_run_len(m, lane), ux = (unsigned)(x0 + lane), uy = (unsigned)y, cx0 = (unsigned)(n_x - 1) - ux;
                row[OBJ_SUM_X] += len * ux + len * (len - 1u) / 2u;
                row[OBJ_SUM_Y] += len * uy;
                if (cx0 > row[OBJ_X0]) row[OBJ_X0] = cx0;
                if (ux + len - 1u > row[OBJ_X1]) row[OBJ_X1] = ux + len - 1u;
                if (uy > row[OBJ_Y1]) row[OBJ_Y1] = uy;
            }
        }
    for (unsigned k = 0; k < n && k < (unsigned)max_pieces; ++k) {
        uint32_t *const row = pieces.data() + (size_t)k * OBJ_WORDS;
        row[OBJ_X0] = (unsigned)(n_x - 1) - row[OBJ_X0];
        row[OBJ_Y0] = row[OBJ_FIRST] / (unsigned)n_x;
    }
    if (n != want_n) { printf("mismatch n_pieces at 0 got %u want %u\n", n, want_n); return 0; }
    for (size_t i = 0; i < pieces.size(); ++i)
        if (pieces[i] != want_pieces[i]) { printf("mismatch pieces at %zu got %u want %u\n", i, pieces[i], want_pieces[i]); return 0; }
    for (size_t i = 0; i < covered.size(); ++i)
        if (covered[i] != want_cov[i]) { printf("mismatch covered at %zu got %u want %u\n", i, covered[i], want_cov[i]); return 0; }
    printf("ok pieces %u runs %ld\n", n, runs);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2 || (strcmp(argv[1], "check") && strcmp(argv[1], "match"))) { fprintf(stderr, "usage: obj_match_check check CALL ... | match FILE ...\n"); return 2; }
    for (int i = 2; i < argc; ++i) {
        const int rc = argv[1][0] == 'c' ? check(argv[i]) : match(argv[i]);
        if (rc) return rc;
    }
    return 0;
}
