// cpol_members.inl -- the gate kernel of an ENSEMBLE sweep: one scan geometry, many model states.
//
// Reference functions replaced (wolfidan/cosmo_pol): nothing as a whole -- the reference runs one model state per
// process.  Per member the kernel is get_all_radar_pts / trilinear_interp (interpolation/interpolation_c.c:12-164) and the
// mask coding (interpolation/interpolation.py:398-411), as cpol_interp.inl restates them.
//
// The members of an ensemble (cpol_stage_member) share the grid and the level heights, so everything of a sub-beam gate that
// does not read the cube V is the same for all of them: the ray path, the geodesic, the rotated-pole transform, the cell
// index and fractions, the level search in the four height columns -- the float64 work that bounds k_interp_sweep.
// k_interp_members (cpol_interp.inl) computes that ONCE per sub-beam gate -- it IS interp_gate, the device function of
// k_interp_sweep, instantiated with MEMBERS = true: the same statements up to and including gate_geometry, in the same forms
// for the same launch, hence the same bits -- and then walks the requested members (members_values below): 8 neighbour gathers
// per four variables, the vertical interpolation and the blend, statement by statement gate_value4's.
// (interp_gate is switched at compile time, not cut into a geometry and a values function that both kernels call: cut that way,
// the register allocation of the existing kernels moved -- k_interp_export 127 -> 129 VGPRs and 4 -> 3 wavefronts per SIMD,
// k_interp_sweep 127 -> 119 -- while `if constexpr` leaves their code as it was: profiles/ensemble_resource_usage.txt.)
// This file is included by cpol_interp.inl in front of interp_gate.
//
// LAYOUT of the work arrays: member mm of the call is the block of rows [mm * n_rays, (mm + 1) * n_rays) of a sweep of
// n_members * n_rays rays -- vals[v][mm][ray][sub][gate], mask / elev[mm][ray][sub][gate] -- which is exactly what the second
// half of the launch sequence reads for such a sweep.  A wavefront is 64 consecutive gates of one (ray, sub-beam): every
// store instruction of it writes 256 contiguous bytes (64 for the mask), whole 128-byte lines when n_gates is a multiple of 32.
//
// LOADS IN FLIGHT: the walk is over (member, group of four variables) pairs; the 8 x 16-byte gathers of the NEXT pair are
// issued before the current pair is interpolated and stored (the stores may alias the cube as far as the compiler knows, so
// the loads stay where they are written), one pair of 32 VGPRs ahead.
//
// TIMED (k_interp_timed, cpol_ray_tables_t.time_blend): ONE scan whose ray r reads the state mb.V[ray_state[r]] blended with
// the next one of the series by the ray's weight w (timed_blend below, the host rule of cosmo_pol_amd/timeline.py: three float32
// operations, the -9999 sentinel kept, w == 0 reads the earlier state alone).  The blend is applied to the eight neighbour
// values before the vertical interpolation, so the statements behind it are member_blend4's on blended operands: the bits of
// a sweep over the host-blended cube.  A wavefront is 64 gates of one ray: the state index, the weight and the w == 0 branch
// are wave-uniform.  Stores go to the ordinary sweep layout (ONE block of n_rays rows, whatever the number of cubes listed).
// The walk requests both cubes' 16 gathers of a group together (64 VGPRs) and keeps no group ahead.

#ifndef CPOL_MEMBERS_PER_CALL
#define CPOL_MEMBERS_PER_CALL 64      // cube pointers travel as a kernel argument
#endif

struct MemberArgs {
    const float *V[CPOL_MEMBERS_PER_CALL];  // the cube of every requested member, in the order of the call
    int n_members;
    long n_sbg1;                            // sub-beam gates of ONE member (n_rays * n_sub * n_gates)
};

// the per-ray bracket of a timed sweep (device copies of cpol_ray_tables_t.ray_state / ray_weight, validated on the host)
struct TimedArgs {
    const int *ray_state;                   // [n_rays] index into MemberArgs.V of the earlier state
    const float *ray_weight;                // [n_rays] weight of the later state, 0 <= w < 1
};

// one value of the time blend, w != 0 (timeline.blend_states): a + w * (b - a) in three float32 operations (the TU is built with
// -ffp-contract=off: no FMA), the sentinel of either side kept
__device__ __forceinline__ float timed_blend(float a, float b, float w)
{
    const float r = a + w * (b - a);
    return (a == -9999.0f || b == -9999.0f) ? -9999.0f : r;
}

// the 8 neighbours of four consecutive variables: the loads of gate_value4
__device__ __forceinline__ void member_load4(const float *__restrict__ V, int nz, int n_vars, const GateGeom &g, int v0,
                                             F4 a[4], F4 b[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float *p = V + ((g.cell[k] * nz + g.c1[k]) * n_vars + v0);
        a[k] = *(const F4 *)p;
        b[k] = *(const F4 *)(p + n_vars);
    }
}

// ... and its arithmetic (interpolation_c.c:151, 162), operand by operand
__device__ __forceinline__ void member_blend4(const GateGeom &g, float h, const F4 a[4], const F4 b[4], float out[4])
{
    float val[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float dh = h - g.z2[k];
#if CPOL_DIV_AS_PRODUCT
#pragma unroll
        for (int j = 0; j < 4; ++j) val[k][j] = b[k].v[j] - div32_by(b[k].v[j] - a[k].v[j], g.rz[k]) * dh;
#else
        const float dz = g.z1[k] - g.z2[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) val[k][j] = b[k].v[j] - (b[k].v[j] - a[k].v[j]) / dz * dh;
#endif
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        out[j] = g.dx * g.dy * val[0][j] + g.x * val[2][j] * g.dy + g.dx * val[1][j] * g.y
                 + g.x * g.y * val[3][j];
}

// a gate without values, for every member: mask code, NaN in every variable, the elevation
// (n_members blocks of n_sbg1 rows: the members of an ensemble call; ONE block for a timed sweep)
__device__ __forceinline__ void members_fill(const ModelDev &m, const InterpArgs &a, int n_members, long n_sbg1, long sbg,
                                             int code, float elev, float c_lat, float c_lon)
{
    const float qnan = __builtin_nanf("");
    const long n_all = n_sbg1 * n_members;
    for (int mm = 0; mm < n_members; ++mm) {
        const long row = (long)mm * n_sbg1 + sbg;
        a.mask[row] = (signed char)code;
        for (int v = 0; v < m.n_vars; ++v) a.vals[(long)v * n_all + row] = qnan;
        a.elev[row] = elev;
        if (a.coords) { a.coords[2 * row] = c_lat; a.coords[2 * row + 1] = c_lon; }
    }
}

// one variable of a timed gate: gate_value on the blended neighbours (the tail of a variable count that is no multiple of four)
__device__ __forceinline__ float timed_value(const ModelDev &m, const float *__restrict__ Vlo, const float *__restrict__ Vhi, float w,
                                             const GateGeom &g, float h, int v)
{
    float val[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long at = (g.cell[k] * m.nz + g.c1[k]) * m.n_vars + v;
        float v1 = Vlo[at], v2 = Vlo[at + m.n_vars];
        if (w != 0.0f) {                                // (wave-uniform)
            v1 = timed_blend(v1, Vhi[at], w);
            v2 = timed_blend(v2, Vhi[at + m.n_vars], w);
        }
#if CPOL_DIV_AS_PRODUCT
        val[k] = v2 - div32_by(v2 - v1, g.rz[k]) * (h - g.z2[k]);
#else
        val[k] = v2 - (v2 - v1) / (g.z1[k] - g.z2[k]) * (h - g.z2[k]);
#endif
    }
    return g.dx * g.dy * val[0] + g.x * val[2] * g.dy + g.dx * val[1] * g.y + g.x * g.y * val[3];
}

// the values of a gate inside the horizontal domain, for every member (g: gate_geometry's result; e32 not yet folded)
// TIMED: for the one row of the gate, from the states mb.V[lo] and mb.V[lo + 1] blended by w (w == 0: mb.V[lo] alone)
template <bool TIMED = false>
__device__ __forceinline__ void members_values(const ModelDev &m, const InterpArgs &a, const MemberArgs &mb, const GateGeom &g,
                                               long sbg, float h32, float e32, float rlat, float rlon, int lo = 0, float w = 0.0f)
{
    const float qnan = __builtin_nanf("");
    const int n_blocks = TIMED ? 1 : mb.n_members;
    const long n_all = mb.n_sbg1 * n_blocks;
    // elevation folded into [0, 90] for the LUT (doppler_scatter.py:173-176)
    if (e32 > 90.0f) e32 = 180.0f - e32;
    if (e32 < 0.0f) e32 = -e32;
    if (g.status != 0) {                                // above the model top / below the topography: the heights decide, for every member
        members_fill(m, a, n_blocks, mb.n_sbg1, sbg, g.status, e32, rlat, rlon);
        return;
    }
    const int nz = m.nz, n_vars = m.n_vars;
    const int n_grp = n_vars >> 2;                      // groups of four variables (wave-uniform)
    // what is left of a member behind its groups: the last n_vars % 4 variables, the mask off variable 0 (the sentinel and bad-value
    // pinning: -9999 -> +1, NaN -> -1, then NaN in every variable), the elevation
    auto finish = [&](int mm, float v0) {
        const long row = (long)mm * mb.n_sbg1 + sbg;
        ModelDev mv = m;
        mv.V = mb.V[TIMED ? lo : mm];
        for (int v = n_grp * 4; v < n_vars; ++v) {
            float o;
            if constexpr (TIMED) o = timed_value(m, mv.V, mb.V[w != 0.0f ? lo + 1 : lo], w, g, h32, v);
            else o = gate_value(mv, g, h32, v);
            if (v == 0) v0 = o;
            a.vals[(long)v * n_all + row] = o;
        }
        int status = 0;
        if (v0 == -9999.0f) status = 1;
        else if (!(v0 == v0)) status = -1;
        if (status != 0)
            for (int v = 0; v < n_vars; ++v) a.vals[(long)v * n_all + row] = qnan;
        a.mask[row] = (signed char)status;
        a.elev[row] = e32;
        if (a.coords) { a.coords[2 * row] = rlat; a.coords[2 * row + 1] = rlon; }
    };
    if (n_grp == 0) {
        for (int mm = 0; mm < n_blocks; ++mm) finish(mm, 0.0f);
        return;
    }
    if constexpr (TIMED) {
        const float *const Vlo = mb.V[lo], *const Vhi = mb.V[w != 0.0f ? lo + 1 : lo];
        float v0 = 0.0f;
        for (int grp = 0; grp < n_grp; ++grp) {
            F4 ca[4], cb[4];
            member_load4(Vlo, nz, n_vars, g, grp * 4, ca, cb);
            if (w != 0.0f) {                            // (wave-uniform) the later state's gathers beside the earlier one's
                F4 da[4], db[4];
                member_load4(Vhi, nz, n_vars, g, grp * 4, da, db);
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ca[k].v[j] = timed_blend(ca[k].v[j], da[k].v[j], w);
                        cb[k].v[j] = timed_blend(cb[k].v[j], db[k].v[j], w);
                    }
            }
            float o[4];
            member_blend4(g, h32, ca, cb, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) a.vals[(long)(grp * 4 + j) * n_all + sbg] = o[j];
            if (grp == 0) v0 = o[0];
        }
        finish(0, v0);
        return;
    }
    F4 ca[4], cb[4];
    member_load4(mb.V[0], nz, n_vars, g, 0, ca, cb);
    const int total = mb.n_members * n_grp;
    int mm = 0, grp = 0;
    float v0 = 0.0f;
#pragma unroll 2
    for (int it = 0; it < total; ++it) {
        int nm = mm, ngrp = grp + 1;
        if (ngrp == n_grp) { ngrp = 0; nm = mm + 1; }
        F4 na[4], nb[4];
        if (it + 1 < total) {                           // (wave-uniform) the next pair's gathers, in flight over this pair's arithmetic
            member_load4(mb.V[nm], nz, n_vars, g, ngrp * 4, na, nb);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { na[k] = ca[k]; nb[k] = cb[k]; }
        }
        float o[4];
        member_blend4(g, h32, ca, cb, o);
        const long row = (long)mm * mb.n_sbg1 + sbg;
#pragma unroll
        for (int j = 0; j < 4; ++j) a.vals[(long)(grp * 4 + j) * n_all + row] = o[j];
        if (grp == 0) v0 = o[0];
        if (ngrp == 0) finish(mm, v0);                  // (the member's last group)
#pragma unroll
        for (int k = 0; k < 4; ++k) { ca[k] = na[k]; cb[k] = nb[k]; }
        mm = nm; grp = ngrp;
    }
}
