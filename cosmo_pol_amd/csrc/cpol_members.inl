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

#ifndef CPOL_MEMBERS_PER_CALL
#define CPOL_MEMBERS_PER_CALL 64      // cube pointers travel as a kernel argument
#endif

struct MemberArgs {
    const float *V[CPOL_MEMBERS_PER_CALL];  // the cube of every requested member, in the order of the call
    int n_members;
    long n_sbg1;                            // sub-beam gates of ONE member (n_rays * n_sub * n_gates)
};

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
__device__ __forceinline__ void members_fill(const ModelDev &m, const InterpArgs &a, const MemberArgs &mb, long sbg,
                                             int code, float elev, float c_lat, float c_lon)
{
    const float qnan = __builtin_nanf("");
    const long n_all = mb.n_sbg1 * mb.n_members;
    for (int mm = 0; mm < mb.n_members; ++mm) {
        const long row = (long)mm * mb.n_sbg1 + sbg;
        a.mask[row] = (signed char)code;
        for (int v = 0; v < m.n_vars; ++v) a.vals[(long)v * n_all + row] = qnan;
        a.elev[row] = elev;
        if (a.coords) { a.coords[2 * row] = c_lat; a.coords[2 * row + 1] = c_lon; }
    }
}

// the values of a gate inside the horizontal domain, for every member (g: gate_geometry's result; e32 not yet folded)
__device__ __forceinline__ void members_values(const ModelDev &m, const InterpArgs &a, const MemberArgs &mb, const GateGeom &g,
                                               long sbg, float h32, float e32, float rlat, float rlon)
{
    const float qnan = __builtin_nanf("");
    const long n_all = mb.n_sbg1 * mb.n_members;
    // elevation folded into [0, 90] for the LUT (doppler_scatter.py:173-176)
    if (e32 > 90.0f) e32 = 180.0f - e32;
    if (e32 < 0.0f) e32 = -e32;
    if (g.status != 0) {                                // above the model top / below the topography: the heights decide, for every member
        members_fill(m, a, mb, sbg, g.status, e32, rlat, rlon);
        return;
    }
    const int nz = m.nz, n_vars = m.n_vars;
    const int n_grp = n_vars >> 2;                      // groups of four variables (wave-uniform)
    // what is left of a member behind its groups: the last n_vars % 4 variables, the mask off variable 0 (the sentinel and bad-value
    // pinning: -9999 -> +1, NaN -> -1, then NaN in every variable), the elevation
    auto finish = [&](int mm, float v0) {
        const long row = (long)mm * mb.n_sbg1 + sbg;
        ModelDev mv = m;
        mv.V = mb.V[mm];
        for (int v = n_grp * 4; v < n_vars; ++v) {
            const float o = gate_value(mv, g, h32, v);
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
        for (int mm = 0; mm < mb.n_members; ++mm) finish(mm, 0.0f);
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
