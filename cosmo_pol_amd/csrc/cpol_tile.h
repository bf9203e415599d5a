// cpol_tile.h -- k_gate1_ray's tiles: which rays and gates a workgroup takes (device), and how many workgroups the
// launch has (host).  Plain C++ without HIP types, so that a host test can include it and walk every block.
//
// A wavefront of k_gate1_ray is one species on a tile of R neighbouring rays x G gates (R x G = 64), not on 64 gates of
// ONE ray: neighbouring rays at the same range have nearly the same T and PSD slope, hence the same (slice, panel) block
// of the integral table, and the lanes' gathers of a block coalesce in TA / L1.  Lane l takes gate (l mod G) of ray
// (l / G) of the tile: G consecutive gates of a row are consecutive lanes.
//
// Workgroup -> tile, from the linear block index b.  The hardware deals workgroups to the 8 XCDs round robin by b, so
// b mod 8 names the blocks that share an XCD's L2 (not WHICH XCD).  The unit dealt to an XCD class is a "super tile" of
// R rays x 32 gates (S = 32 / G gate tiles; one tile if G >= 32), 32-gate aligned:
//   - every XCD gets every range: the super tiles are numbered ray tile fastest (s = column * TR + ray tile), and XCD
//     class x takes s = x, x + 8, ...  (the ranges differ threefold in work: no hydrometeor in the first kilometres, the
//     melting layer further out; tools/gate1_trace.py shows every XCD ending within 2 us);
//   - the narrow row segments of the S tiles of a super tile (G x 4 B per row and output) are written from one L2.  Where
//     a row is a multiple of 128 B long, every 128-B line of an output is written from one XCD; otherwise (c2: 2000-B
//     rows) a line straddling two super tiles is shared by two.  Dealing whole ray tiles instead (every line on one XCD
//     but at ray-tile boundaries) measured no better on c2 and balances worse (profiles/r7_variants.txt).
// b = 8 k + x  ->  super tile s = 8 (k / S) + x, member k mod S.  The grid is padded to whole super tiles and to a
// multiple of 8 of them; a block whose tile lies beyond the sweep leaves at once.
#pragma once

#if defined(__HIPCC__)
#define CPOL_TILE_HD __host__ __device__ __forceinline__
#else
#define CPOL_TILE_HD inline
#endif

#ifndef CPOL_GATE1_TILE_GATES_LOG2
#define CPOL_GATE1_TILE_GATES_LOG2 4       // k_gate1_ray: a wavefront = (64 >> this) rays x (1 << this) gates (6: 64 gates of one ray;
                                           // c2: 4 x 16 and 8 x 8 ahead of 16 x 4 and 32 x 2, profiles/r7_variants.txt)
#endif
static_assert(CPOL_GATE1_TILE_GATES_LOG2 >= 0 && CPOL_GATE1_TILE_GATES_LOG2 <= 6, "a tile holds 64 lanes");

struct Gate1Tiles {
    int tr, tg;        // ray tiles, gate tiles of the sweep
    int per_super;     // gate tiles of a super tile
    int n_super;       // super tiles: tr x ceil(tg / per_super)
    int n_blocks;      // the grid: 8 x ceil(n_super / 8) x per_super
};

CPOL_TILE_HD Gate1Tiles gate1_tiles(int n_rays, int n_gates)
{
    constexpr int TG = CPOL_GATE1_TILE_GATES_LOG2, G = 1 << TG, R = 64 >> TG;
    Gate1Tiles t;
    t.tr = (n_rays + R - 1) / R;
    t.tg = (n_gates + G - 1) / G;
    t.per_super = G >= 32 ? 1 : 32 / G;
    t.n_super = t.tr * ((t.tg + t.per_super - 1) / t.per_super);
    t.n_blocks = (t.n_super + 7) / 8 * 8 * t.per_super;
    return t;
}

// the first ray and gate of block b's tile; false: a block of the padding (no gate of the sweep)
CPOL_TILE_HD bool gate1_tile_of_block(const Gate1Tiles &t, unsigned b, int &ray0, int &gate0)
{
    constexpr int TG = CPOL_GATE1_TILE_GATES_LOG2, G = 1 << TG, R = 64 >> TG;
    const unsigned x = b & 7u, k = b >> 3;
    const unsigned s = (k / (unsigned)t.per_super) * 8u + x;
    if (s >= (unsigned)t.n_super) return false;
    const int rt = (int)(s % (unsigned)t.tr), col = (int)(s / (unsigned)t.tr);
    const int gt = col * t.per_super + (int)(k % (unsigned)t.per_super);
    if (gt >= t.tg) return false;
    ray0 = rt * R;
    gate0 = gt * G;
    return true;
}

// lane -> (ray, gate) inside the tile
CPOL_TILE_HD void gate1_lane_in_tile(int lane, int &dray, int &dgate)
{
    constexpr int TG = CPOL_GATE1_TILE_GATES_LOG2;
    dray = lane >> TG;
    dgate = lane & ((1 << TG) - 1);
}
