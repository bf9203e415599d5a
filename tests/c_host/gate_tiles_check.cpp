// Host check of k_gate1_ray's workgroup -> tile decode (cosmo_pol_amd/csrc/cpol_tile.h), built once per tile shape
// with -DCPOL_GATE1_TILE_GATES_LOG2=<k>.  For every sweep shape given on the command line (rays gates pairs):
//   - (block, lane) -> (ray, gate) covers every gate of the sweep exactly once, and nothing outside it;
//   - every 32-gate-aligned segment of a row is written by blocks of ONE XCD class (block mod 8); where the row is a
//     multiple of 32 gates, so is every 128-B line of a [ray][gate] float32 output and of the float64 RVEL;
//   - the XCD classes hold equal numbers of super tiles, give or take one.
// Prints GATE_TILES_OK on success.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cpol_tile.h"

// elements [l, l + per_line) of the flat [ray][gate] index (per_line = 32: a 128-B line of float32, 16: of float64), or
// the 32-gate segments of every row (rows = true): written from one XCD class each
static int one_class(int n_rays, int n_gates, const std::vector<int> &cls, int per_line, bool rows)
{
    for (int r = 0; r < (rows ? n_rays : 1); ++r) {
        const long base = rows ? (long)r * n_gates : 0, n = rows ? n_gates : (long)n_rays * n_gates;
        for (long l0 = 0; l0 < n; l0 += per_line) {
            const long l1 = l0 + per_line < n ? l0 + per_line : n;
            for (long q = l0 + 1; q < l1; ++q)
                if (cls[base + q] != cls[base + l0]) {
                    printf("%d x %d: %s at %ld written from XCD classes %d and %d\n", n_rays, n_gates, rows ? "row segment" : "line",
                           base + l0, cls[base + l0], cls[base + q]);
                    return 1;
                }
        }
    }
    return 0;
}

static int check(int n_rays, int n_gates)
{
    const Gate1Tiles t = gate1_tiles(n_rays, n_gates);
    std::vector<int> seen((size_t)n_rays * n_gates, 0), cls((size_t)n_rays * n_gates, -1);
    long supers[8] = {0};
    if (t.n_blocks % 8 != 0) { printf("n_blocks %d not a multiple of 8\n", t.n_blocks); return 1; }
    for (int b = 0; b < t.n_blocks; ++b) {
        int ray0 = -1, gate0 = -1;
        if (!gate1_tile_of_block(t, (unsigned)b, ray0, gate0)) continue;
        if (ray0 < 0 || ray0 >= n_rays || gate0 < 0 || gate0 >= n_gates) {
            printf("%d x %d: block %d starts outside the sweep (%d, %d)\n", n_rays, n_gates, b, ray0, gate0);
            return 1;
        }
        if (gate0 % 32 == 0) supers[b & 7] += 1;
        for (int lane = 0; lane < 64; ++lane) {
            int dr, dg;
            gate1_lane_in_tile(lane, dr, dg);
            const int r = ray0 + dr, g = gate0 + dg;
            if (r >= n_rays || g >= n_gates) continue;
            seen[(size_t)r * n_gates + g] += 1;
            cls[(size_t)r * n_gates + g] = b & 7;
        }
    }
    for (size_t q = 0; q < seen.size(); ++q)
        if (seen[q] != 1) {
            printf("%d x %d: gate (%ld, %ld) taken %d times\n", n_rays, n_gates, (long)(q / n_gates), (long)(q % n_gates), seen[q]);
            return 1;
        }
    if (one_class(n_rays, n_gates, cls, 32, true)) return 1;
    if (n_gates % 32 == 0 && (one_class(n_rays, n_gates, cls, 32, false) || one_class(n_rays, n_gates, cls, 16, false))) return 1;
    long lo = supers[0], hi = supers[0];
    for (int x = 1; x < 8; ++x) { lo = supers[x] < lo ? supers[x] : lo; hi = supers[x] > hi ? supers[x] : hi; }
    if (hi - lo > 1) { printf("%d x %d: super tiles per XCD class %ld .. %ld\n", n_rays, n_gates, lo, hi); return 1; }
    return 0;
}

int main(int argc, char **argv)
{
    for (int k = 1; k + 1 < argc; k += 2)
        if (check(atoi(argv[k]), atoi(argv[k + 1]))) return 1;
    printf("GATE_TILES_OK\n");
    return 0;
}
