// cpol_place.h -- where the kernels of a call write each output array and how it reaches the caller: the placement rule of
// run_sequence (cosmo_pol_hip.hip) for the sweep's own arrays, the superobservations and the ensemble statistics alike,
// decided once per call by place_outputs() from plain numbers.  Plain C++ without HIP types, so that a host test can include
// it (tests/c_host/place_check.cpp, tests/test_place_cpu.py pin the rule without a GPU).  The caller's addresses come in as
// integers; kinds and offsets go out, never device pointers: run_sequence adds the bases and owns every buffer.
#pragma once

#include <cstddef>
#include <cstdint>

enum { PLACE_SWEEP = 0, PLACE_SUPEROB, PLACE_STATS, PLACE_PRODUCTS };      // the product an array belongs to
// not written; written through the caller's (device) pointer; at `offset` + win_skew into the device image of the caller's pinned
// window; at `offset` into a buffer of the context -- the sweep's arrays each into a grow-only buffer of their own (offset 0: the
// debug reads and the test hooks read those), the other products packed into one block per product
enum { PLACE_NONE = 0, PLACE_IN_PLACE, PLACE_WINDOW, PLACE_OWN };
constexpr int PLACE_MAX_ARRAYS = 128;
constexpr int PLACE_MAX_COPIES = PLACE_MAX_ARRAYS + 32;
constexpr size_t PLACE_PAD = 256;              // every array of a packed block starts at a multiple of it

struct PlaceArray {
    uintptr_t user = 0;            // the caller's pointer (0: not asked for)
    size_t bytes = 0;
    bool produced = false;         // the call makes it
    int product = PLACE_SWEEP;
    bool own_under_debug = false;  // never written in place while the debug reads are on (sz_total: they read the context's copy)
    // a `count` array: `rows` rows of bytes / rows each (0: one piece).  Out of a buffer of the context only the rows in row_mask are
    // copied, the others are not the caller's to be written; in a window image the kernel zeroes them instead (zero_rest)
    int rows = 0;
    uint32_t row_mask = 0;
};

struct PlaceWhere { int kind = PLACE_NONE; size_t offset = 0; };
struct PlaceCopy { int array; size_t offset, bytes; };     // `bytes` at `offset` of the array, from where it was placed to the caller's

struct PlacePlan {
    // pinned-host mode: when the requested arrays lie in one window of the caller's slab (only alignment padding between them) the
    // kernels write into a device image of that window and ONE device-to-host copy moves it, [win_lo, win_hi) from win_skew on
    // (instead of up to 18 copies of a few hundred KB each)
    bool window = false;
    uintptr_t win_lo = 0, win_hi = 0;
    size_t win_skew = 0, win_bytes = 0;                    // win_bytes: what the image needs
    PlaceWhere where[PLACE_MAX_ARRAYS];
    size_t block_bytes[PLACE_PRODUCTS] = {0, 0, 0};        // the packed blocks (the sweep's arrays have none)
    int n_copies = 0;                                      // what neither lies in the window nor was written in place
    PlaceCopy copies[PLACE_MAX_COPIES];
};

// outputs_on_device: 0 blocking host arrays, 1 device arrays, 2 pinned host arrays (no wait); n <= PLACE_MAX_ARRAYS
inline void place_outputs(const PlaceArray *a, int n, int outputs_on_device, bool debug_reads, PlacePlan *pl)
{
    const bool dev = outputs_on_device == 1;
    // (the sweep's kernels need their arrays whether or not the caller asks for them; the other products write what is asked for)
    const auto made = [&](int i) { return a[i].produced && (a[i].user || a[i].product == PLACE_SWEEP); };
    size_t sum = 0;
    if (outputs_on_device == 2 && !debug_reads)
        for (int i = 0; i < n; ++i) {
            if (!a[i].produced || !a[i].user) continue;
            if (!pl->win_lo || a[i].user < pl->win_lo) pl->win_lo = a[i].user;
            if (!pl->win_hi || a[i].user + a[i].bytes > pl->win_hi) pl->win_hi = a[i].user + a[i].bytes;
            sum += a[i].bytes;
        }
    pl->window = pl->win_lo && (size_t)(pl->win_hi - pl->win_lo) <= sum + sum / 4 + 4096;
    // (the device image keeps the window's alignment modulo 64 B, so that every array of the image is aligned exactly like its
    // host counterpart: a float32 array at an address 4 mod 8 followed by a float64 array must not shift the latter to a
    // misaligned device address)
    pl->win_skew = pl->window ? (size_t)(pl->win_lo & 63) : 0;
    pl->win_bytes = pl->window ? (size_t)(pl->win_hi - pl->win_lo) + 64 : 0;
    for (int i = 0; i < n; ++i) {
        PlaceWhere &w = pl->where[i];
        w = PlaceWhere{};
        if (!made(i)) continue;
        if (dev && a[i].user && !(debug_reads && a[i].own_under_debug)) { w.kind = PLACE_IN_PLACE; continue; }
        if (pl->window && a[i].user) { w.kind = PLACE_WINDOW; w.offset = (size_t)(a[i].user - pl->win_lo); continue; }
        w.kind = PLACE_OWN;
        if (a[i].product != PLACE_SWEEP) {
            w.offset = pl->block_bytes[a[i].product];
            pl->block_bytes[a[i].product] += (a[i].bytes + PLACE_PAD - 1) & ~(PLACE_PAD - 1);
        }
        if (!a[i].user) continue;
        if (a[i].rows == 0) { pl->copies[pl->n_copies++] = PlaceCopy{i, 0, a[i].bytes}; continue; }
        const size_t row = a[i].bytes / (size_t)a[i].rows;
        for (int r = 0; r < a[i].rows; ++r)
            if ((a[i].row_mask >> r) & 1u) pl->copies[pl->n_copies++] = PlaceCopy{i, r * row, row};
    }
}
