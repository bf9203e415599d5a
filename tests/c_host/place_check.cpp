// Host check of the placement plan (cosmo_pol_amd/csrc/cpol_place.h); tests/test_place_cpu.py drives it.
//   place_check MODE DEBUG ARRAY ...   MODE: outputs_on_device 0 / 1 / 2; DEBUG: the debug reads 0 / 1; one ARRAY per output array of
//                                      the call, user:bytes:produced:product:own_under_debug:rows:row_mask (user and row_mask in hex)
// prints the plan, one record per line:
//   window W lo hi skew bytes          (lo, hi in hex)
//   block PRODUCT bytes
//   where INDEX kind offset
//   copy ARRAY offset bytes
#include <cstdio>
#include <cstdlib>
#include "cpol_place.h"

int main(int argc, char **argv)
{
    if (argc < 3 || argc - 3 > PLACE_MAX_ARRAYS) { fprintf(stderr, "usage: place_check MODE DEBUG ARRAY ...\n"); return 2; }
    const int mode = atoi(argv[1]), n = argc - 3;
    const bool debug = atoi(argv[2]) != 0;
    PlaceArray *const a = new PlaceArray[n];
    for (int i = 0; i < n; ++i) {
        unsigned long long user = 0, bytes = 0;
        unsigned mask = 0;
        int produced = 0, product = 0, own = 0, rows = 0;
        if (sscanf(argv[3 + i], "%llx:%llu:%d:%d:%d:%d:%x", &user, &bytes, &produced, &product, &own, &rows, &mask) != 7) {
            fprintf(stderr, "bad array '%s'\n", argv[3 + i]);
            return 2;
        }
        a[i].user = (uintptr_t)user; a[i].bytes = (size_t)bytes; a[i].produced = produced != 0; a[i].product = product;
        a[i].own_under_debug = own != 0; a[i].rows = rows; a[i].row_mask = mask;
    }
    PlacePlan *const pl = new PlacePlan;
    place_outputs(a, n, mode, debug, pl);
    printf("window %d %llx %llx %zu %zu\n", (int)pl->window, (unsigned long long)pl->win_lo, (unsigned long long)pl->win_hi, pl->win_skew, pl->win_bytes);
    for (int q = 0; q < PLACE_PRODUCTS; ++q) printf("block %d %zu\n", q, pl->block_bytes[q]);
    for (int i = 0; i < n; ++i) printf("where %d %d %zu\n", i, pl->where[i].kind, pl->where[i].offset);
    for (int c = 0; c < pl->n_copies; ++c) printf("copy %d %zu %zu\n", pl->copies[c].array, pl->copies[c].offset, pl->copies[c].bytes);
    delete pl;
    delete[] a;
    return 0;
}
