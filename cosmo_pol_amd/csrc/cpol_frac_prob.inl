// cpol_frac_prob.inl -- neighbourhood ensemble probabilities: NEP, NMEP, the sums of the ensemble FSS and the reliability table
// of the blocks (members) of one scored finishing call (cpol_fraction_probabilities, pointed to by cpol_fractions_ensemble.probabilities).
//
// Reference functions replaced (wolfidan/cosmo_pol): none -- its users pull every member's map to the host and box-filter it there.
// The rule is the one of include/cosmo_pol_amd.h and cosmo_pol_amd/neighbourhood.py (`ensemble_sums`):
//
// THE RULE
// Inputs are those of cpol_fractions, unchanged.  F[b][t], O[t], NF[b][t][w][y][x] and NO[t][w][y][x] are the binary maps and
// clipped window counts defined there.  M = n_blocks; in an ensemble call a block is a member.
// Per threshold t, radius index w and cell:
//   S[t][w][y][x] = sum over b of NF[b][t][w][y][x] (uint32).  NEP is S / (M * window_cells); the division is the host's.
//   A[t][w][y][x] = #{ b : NF[b][t][w][y][x] > 0 } (uint32, 0 ... M).  NMEP is A / M.
//   OA[t][w][y][x] = NO[t][w][y][x] > 0.
// Both maps are written for EVERY cell of the grid.  The domain only decides which cells are set and which cells are summed.
// Sums over the cells of the domain, uint64:
//   prob_sums[t][w][3] = (diff2, forecast2, observed2): diff2 = sum (S - M * NO)^2, forecast2 = sum S^2, observed2 = M^2 * sum
//   NO^2.  neighbourhood.fss applied to these three gives the ensemble FSS unchanged.  With M == 1 they equal block 0's row of
//   `sums`.
//   reliability[t][w][k][o], k = 0 ... M, o = 0 | 1: the number of domain cells with A == k and OA == o.  At radius 0 this is the
//   classic table "k of M members exceed, observed yes or no".  At larger radii it is the NMEP against the neighbourhood-maximum
//   observation.  Every [t][w] slice sums to n_domain.
// Limits are conditions, not measurements (frac_prob_check, cpol_frac.h): 1 <= n_blocks <= 256; with c = min(2 * r_max + 1, n_y)
// * min(2 * r_max + 1, n_x), M * c < 2^32 and n_y * n_x * (M * c)^2 < 2^64.  |S - M * NO| <= M * c, so the bound covers all
// three sums.
// The result depends neither on the order of the blocks nor on how the work is cut.
//
// One launch directly behind k_frac_score, which has left the summed-area tables of every block and of the observation in a.sat:
// k_frac_members reads only those tables and the domain.  Every number is an integer; no float arithmetic, no compare-and-swap
// loops, no workgroup waits on another; the atomics are integer additions -- uint32 in LDS for the reliability table, 64-bit in
// global memory, one per sum and workgroup and one per non-zero table entry and workgroup.

struct FracProbArgs {
    FracArgs f;                     // the maps and tables as frac_launch resolved them (sums and totals are not touched)
    unsigned long long *prob_sums;  // [n_thr][n_radii][3]: zero before the launch
    unsigned long long *reliability;    // [n_thr][n_radii][n_blocks + 1][2]: likewise
    unsigned *member_sum;           // [n_thr][n_radii][n_y][n_x] or NULL
    unsigned *member_any;           // likewise
    int n_members;                  // M = n_blocks, 1 ... FRAC_PROB_MAX_BLOCKS
    int table_entries;              // (M + 1) * 2: a [t][w] slice of the table
};

// A workgroup owns FRAC_CELLS consecutive cells of ONE threshold and ONE radius, four per thread, strided so that a wavefront
// reads and writes consecutive cells.  (All radii in one workgroup, as k_frac_score has them, leave 88 workgroups per threshold
// on a 300 x 300 map: too few to cover the latency of the look-ups; DESIGN.md 3.24 has both forms' times.)  Per cell the window
// is clipped once: four offsets serve the observation's table and every block's.  The loop over the blocks carries two integer
// sums and no load depends on them, so the unrolled loop keeps the look-ups of several blocks in flight.  The squares go into
// uint64 registers and leave as in k_frac_score: shuffles inside the wavefront, the four wavefronts through LDS, ONE atomic
// addition per sum and workgroup.  The reliability table of the workgroup's cells is counted in LDS ([M + 1][2] uint32, at most
// 2056 bytes; a workgroup has at most 1024 cells) and its non-zero entries are added to the global table behind a barrier.
// Every lane reaches every barrier.
__global__ __launch_bounds__(FRAC_THREADS) void k_frac_members(const FracProbArgs p)
{
    __shared__ unsigned long long part[FRAC_THREADS / 64][3];
    __shared__ unsigned rel[(FRAC_PROB_MAX_BLOCKS + 1) * 2];
    const FracArgs &a = p.f;
    const int tid = threadIdx.x;
    const int tw = (int)(blockIdx.x / (unsigned)a.score_groups);     // t * n_radii + w
    const int grp = (int)(blockIdx.x % (unsigned)a.score_groups);
    const int t = tw / a.n_radii, r = a.radii[tw - t * a.n_radii];
    const int W = a.n_x + 1;
    const int M = p.n_members;
    const unsigned *const so = a.sat + (a.n_blocks * a.n_thr + t) * a.table;
    const unsigned *const sf0 = a.sat + (long)t * a.table;            // block 0's table of threshold t ...
    const long sf_step = (long)a.n_thr * a.table;                    // ... and block b's lies b steps further
    const bool maps = p.member_sum != nullptr || p.member_any != nullptr;
    for (int e = tid; e < p.table_entries; e += FRAC_THREADS) rel[e] = 0u;
    __syncthreads();
    unsigned long long acc[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int i = 0; i < FRAC_CELLS / FRAC_THREADS; ++i) {
        const int cell = grp * FRAC_CELLS + i * FRAC_THREADS + tid;
        if (cell >= a.cells) continue;
        const bool dom = !a.domain || a.domain[cell] != 0;
        if (!dom && !maps) continue;                  // (outside the domain a cell is only written, never summed)
        const int y = cell / a.n_x, x = cell - y * a.n_x;
        const int y0 = max(y - r, 0), y1 = min(y + r, a.n_y - 1) + 1, x0 = max(x - r, 0), x1 = min(x + r, a.n_x - 1) + 1;
        const int i11 = y1 * W + x1, i01 = y0 * W + x1, i10 = y1 * W + x0, i00 = y0 * W + x0;
        const unsigned no = so[i11] - so[i01] - so[i10] + so[i00];
        unsigned S = 0u, A = 0u;
        const unsigned *sf = sf0;
#pragma unroll 4
        for (int b = 0; b < M; ++b, sf += sf_step) {
            const unsigned nf = sf[i11] - sf[i01] - sf[i10] + sf[i00];
            S += nf;
            A += nf != 0u ? 1u : 0u;
        }
        if (maps) {
            const long at = (long)tw * a.cells + cell;
            if (p.member_sum) p.member_sum[at] = S;
            if (p.member_any) p.member_any[at] = A;
        }
        if (dom) {
            // (M * no <= M * c < 2^32 and |S - M * no| <= M * c: the squares fit 64 bits, frac_prob_check)
            const unsigned long long mo = (unsigned long long)M * no, s = S;
            const unsigned long long d = s > mo ? s - mo : mo - s;
            acc[0] += d * d;
            acc[1] += s * s;
            acc[2] += mo * mo;
            atomicAdd(&rel[(int)A * 2 + (no != 0u ? 1 : 0)], 1u);
        }
    }
    // (every lane of the workgroup arrives here: the shuffles and the barrier need whole wavefronts)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        unsigned long long v = acc[k];
        for (int dlt = 32; dlt > 0; dlt >>= 1) v += __shfl_down(v, dlt);
        if ((tid & 63) == 0) part[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < 3) {
        unsigned long long v = 0ull;
        for (int q = 0; q < FRAC_THREADS / 64; ++q) v += part[q][tid];
        if (v) atomicAdd(&p.prob_sums[(long)tw * 3 + tid], v);
    }
    // the LDS table is the [M + 1][2] slice of threshold t and radius w, entry for entry
    unsigned long long *const slice = p.reliability + (long)tw * p.table_entries;
    for (int e = tid; e < p.table_entries; e += FRAC_THREADS) {
        const unsigned v = rel[e];
        if (v) atomicAdd(&slice[e], (unsigned long long)v);
    }
}
