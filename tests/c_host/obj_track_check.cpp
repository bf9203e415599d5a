// Host check of the track's validation and per-word pieces (cosmo_pol_amd/csrc/cpol_obj.h); tests/test_object_track_cpu.py drives it.
//   obj_track_check check CALL ...   independent calls.  One CALL: key=value,... -- of the maps: nx ny blocks nthr; of the cpol_objects:
//       conn area max; pad (pad_ as it is handed over; default CPOL_OBJ_TRACK; without that bit the struct is a bare cpol_objects or
//       a cpol_objects_match with nothing behind it); of the match inside: np pc cov (0: NULL); of the track: shift (max_shift) pieces
//       (max_pieces) given (1: shifts_in present) gv (the value of every given shift) corr sh tn tp tc (0: NULL correlation, shift,
//       n_pieces, pieces, covered)
//     prints one line per call:
//       refused <reason>
//       ok scratch S track 0 match M
//       ok scratch S track 1 match M pairs P maps T side D words W bits O pieceoff Q piecebytes B corroff C corrbytes Y bitsgrid G
//          corrgrid H slabs L shiftgrid I rows R cellgroups J decode K shiftbytes a n b pieces c covered d given e
//   obj_track_check track FILE ...   FILE: int32 {n_y, n_x, S, dy, dx} (S = -1: the shift (dy, dx) is given), uint8 flags [n_y][n_x] of
//       Ke and of Kl, then the rule's: uint32 correlation [2S + 1][2S + 1] (S >= 0 only), int32 shift [2], uint8 overlap [n_y][n_x]
//       (le' > 0 and ll > 0).  The flags are packed as k_track_bits packs them (a ballot per 64 cells), every counter is formed as
//       k_track_corr cuts the work (slabs of OBJ_TRACK_ROWS rows through obj_track_count), the argmax through obj_track_key as
//       k_track_shift takes it, and the shifted lookup of every cell through obj_track_number as k_track_runs does.
//     prints one line per file:
//       ok shift DY DX cells N
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
    static int32_t shift_sink[2];
    cpol_fractions f;
    memset(&f, 0, sizeof f);
    f.n_thresholds = (int32_t)num("nthr", 1); f.n_radii = 1;
    f.observed = obs_sink; f.sums = sums_sink; f.totals = totals_sink;
    FracPlan fp;
    const char *why = frac_check_maps(&f, (int)num("nx", 3), (int)num("ny", 2), num("blocks", 2), &fp);
    if (why) { printf("fractions refused %s\n", why); return 0; }
    // the library must not read behind what pad_ announces: the heap block has exactly that size, so that the address sanitizer sees
    // any read beyond it
    const long pad = num("pad", CPOL_OBJ_TRACK);
    const bool track = pad >= 0 && (pad & CPOL_OBJ_TRACK), inner = pad > 0 && (pad & 0xFFFF);
    std::vector<char> heap(track ? sizeof(cpol_objects_track) : inner ? sizeof(cpol_objects_match) : sizeof(cpol_objects), 0);
    cpol_objects *const o = (cpol_objects *)heap.data();
    o->connectivity = (int32_t)num("conn", 4); o->min_area = (int32_t)num("area", 1); o->max_objects = (int32_t)num("max", 16);
    o->n_objects = n_sink; o->table = table_sink;
    o->pad_ = (int32_t)pad;
    if (track || inner) {
        cpol_objects_match *const mo = (cpol_objects_match *)heap.data();
        if (num("np", 1)) mo->n_pieces = n_sink;
        if (num("pc", 1)) mo->pieces = table_sink;
        if (num("cov", 1)) mo->covered = u_sink;
    }
    std::vector<int32_t> given;
    if (track) {
        cpol_objects_track *const tr = (cpol_objects_track *)heap.data();
        tr->max_shift = (int32_t)num("shift", 2); tr->max_pieces = (int32_t)num("pieces", 8);
        if (num("given", 0)) {
            given.assign((size_t)(fp.n_blocks > 1 ? fp.n_blocks - 1 : 1) * fp.n_thr * 2, (int32_t)num("gv", 0));
            tr->shifts_in = given.data();
        }
        if (num("corr", 1)) tr->correlation = table_sink;
        if (num("sh", 1)) tr->shift = shift_sink;
        if (num("tn", 1)) tr->n_pieces = n_sink;
        if (num("tp", 1)) tr->pieces = table_sink;
        if (num("tc", 1)) tr->covered = u_sink;
    }
    ObjPlan pl;
    why = obj_check(o, fp, &pl);
    if (why) { printf("refused %s\n", why); return 0; }
    if (!pl.track) { printf("ok scratch %ld track 0 match %d\n", pl.scratch_bytes, (int)pl.match); return 0; }
    printf("ok scratch %ld track 1 match %d pairs %d maps %ld side %d words %d bits %ld pieceoff %ld piecebytes %ld corroff %ld corrbytes %zu "
           "bitsgrid %ld corrgrid %ld slabs %ld shiftgrid %ld rows %ld cellgroups %ld decode %ld shiftbytes %zu n %zu pieces %zu covered %zu "
           "given %zu\n",
           pl.scratch_bytes, (int)pl.match, pl.n_pairs, pl.track_maps, pl.track_side, pl.track_words, pl.track_bits_offset, pl.track_piece_offset,
           pl.track_piece_bytes, pl.track_corr_offset, pl.track_corr_bytes, pl.grid_track_bits, pl.grid_track_corr, pl.track_slabs,
           pl.grid_track_shift, pl.grid_track_rows, pl.grid_track_cells, pl.grid_track_decode, pl.track_shift_bytes, pl.track_n_bytes,
           pl.track_pieces_bytes, pl.track_covered_bytes, pl.shifts_in.size());
    return 0;
}

// k_track_bits: a ballot per 64 cells, the lanes at or beyond n_x unset
static std::vector<unsigned long long> pack(const std::vector<uint8_t> &flag, int n_y, int n_x, int words)
{
    std::vector<unsigned long long> bits((size_t)n_y * words, 0ull);
    for (int y = 0; y < n_y; ++y)
        for (int x0 = 0; x0 < n_x; x0 += 64) {
            unsigned long long m = 0ull;
            for (int lane = 0; lane < 64 && x0 + lane < n_x; ++lane)
                if (flag[(size_t)y * n_x + x0 + lane]) m |= 1ull << lane;
            bits[(size_t)y * words + (x0 >> 6)] = m;
        }
    return bits;
}

static int track(const char *path)
{
    FILE *fh = fopen(path, "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    int32_t head[5];
    if (fread(head, sizeof head, 1, fh) != 1) { fclose(fh); fprintf(stderr, "short file %s\n", path); return 2; }
    const int n_y = head[0], n_x = head[1], S = head[2];
    if (n_y < 1 || n_x < 1 || n_y > FRAC_MAX_SIDE || n_x > FRAC_MAX_SIDE || S < -1 || S > OBJ_TRACK_MAX_SHIFT ||
        abs(head[3]) > OBJ_TRACK_MAX_GIVEN || abs(head[4]) > OBJ_TRACK_MAX_GIVEN) { fclose(fh); fprintf(stderr, "bad head\n"); return 2; }
    const size_t cells = (size_t)n_y * n_x;
    const int side = 2 * (S < 0 ? 0 : S) + 1, words = (n_x + 63) / 64;
    std::vector<uint8_t> ke(cells), kl(cells), want_overlap(cells);
    std::vector<uint32_t> want_corr(S >= 0 ? (size_t)side * side : 0);
    int32_t want_shift[2];
    const bool read = fread(ke.data(), 1, cells, fh) == cells && fread(kl.data(), 1, cells, fh) == cells &&
                      fread(want_corr.data(), 4, want_corr.size(), fh) == want_corr.size() && fread(want_shift, 4, 2, fh) == 2 &&
                      fread(want_overlap.data(), 1, cells, fh) == cells;
    fclose(fh);
    if (!read) { fprintf(stderr, "short file %s\n", path); return 2; }
    int dy = head[3], dx = head[4];
    if (S >= 0) {
        const std::vector<unsigned long long> be = pack(ke, n_y, n_x, words), bl = pack(kl, n_y, n_x, words);
        // k_track_corr: every counter summed over the slabs; k_track_shift: one maximum over the keys
        unsigned long long best = 0ull;
        for (int c = 0; c < side * side; ++c) {
            unsigned n = 0u;
            for (int y0 = 0; y0 < n_y; y0 += OBJ_TRACK_ROWS)
                n += obj_track_count(be.data(), bl.data(), n_y, words, y0, y0 + OBJ_TRACK_ROWS < n_y ? y0 + OBJ_TRACK_ROWS : n_y, c / side - S, c % side - S);
            if (n != want_corr[(size_t)c]) { printf("mismatch correlation at %d got %u want %u\n", c, n, want_corr[(size_t)c]); return 0; }
            const unsigned long long key = obj_track_key(n, c / side - S, c % side - S, S);
            if (key > best) best = key;
        }
        obj_track_unkey(best, S, &dy, &dx);
    }
    if (dy != want_shift[0] || dx != want_shift[1]) { printf("mismatch shift at 0 got %d,%d want %d,%d\n", dy, dx, want_shift[0], want_shift[1]); return 0; }
    // k_track_runs' lookup: a label array in which every set cell of Ke hangs under the first one, whose number is 1
    std::vector<unsigned> L(cells, OBJ_NONE), aux(cells, 0u);
    unsigned first = OBJ_NONE;
    for (size_t i = 0; i < cells; ++i)
        if (ke[i]) { if (first == OBJ_NONE) first = (unsigned)i; L[i] = first; }
    if (first != OBJ_NONE) aux[first] = 1u;
    long n_cells = 0;
    for (int y = 0; y < n_y; ++y)
        for (int x = 0; x < n_x; ++x) {
            const size_t i = (size_t)y * n_x + x;
            const unsigned got = obj_track_number(L.data(), aux.data(), n_x, n_y, y, x, dy, dx) != 0u && kl[i] ? 1u : 0u;
            if (got != want_overlap[i]) { printf("mismatch overlap at %zu got %u want %u\n", i, got, (unsigned)want_overlap[i]); return 0; }
            n_cells += got;
        }
    printf("ok shift %d %d cells %ld\n", dy, dx, n_cells);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2 || (strcmp(argv[1], "check") && strcmp(argv[1], "track"))) { fprintf(stderr, "usage: obj_track_check check CALL ... | track FILE ...\n"); return 2; }
    for (int i = 2; i < argc; ++i) {
        const int rc = argv[1][0] == 'c' ? check(argv[i]) : track(argv[i]);
        if (rc) return rc;
    }
    return 0;
}
