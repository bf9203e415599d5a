"""Ensembles: many model states under one set of scattering tables and one scan geometry.

Replaces in the reference: nothing -- cosmo_pol runs one model state per process (one RadarOperator, one
load_model_file).  The pure host-side pieces live here so that they are testable without a GPU: the check that
the members of an ensemble really are states of one model (same variables, shape, grid and level heights: what
lets the gate kernel share the geometry, cpol_members.inl), and the planner that cuts a member list into chunks
whose work buffers fit a memory budget.  The operator's entry points are in radar_operator.py."""
import numpy as np

from ._native import MEMBERS_PER_CALL

PROJ_KEYS = ('Lo1', 'La1', 'Lo2', 'La2', 'Latitude_of_southern_pole', 'Longitude_of_southern_pole')


def check_members(members):
    """members: [{'data': {name: [nz, ny, nx]}, 'zlevels', 'proj_info', 'resolution'}, ...] -- raises ValueError
    naming the first member that differs from member 0, and what differs."""
    if len(members) < 2:
        raise ValueError('an ensemble needs at least two members, got %d (member 0 alone is load_model_arrays)'
                         % len(members))
    ref = members[0]
    names = sorted(ref['data'])
    z0 = np.asarray(ref['zlevels'])
    for i, m in enumerate(members):
        if sorted(m['data']) != names:
            diff = sorted(set(names) ^ set(m['data']))
            raise ValueError('ensemble member %d: variable set differs from member 0 (%s)' % (i, ', '.join(diff)))
        for k in names:
            if np.shape(m['data'][k]) != z0.shape:
                raise ValueError('ensemble member %d: variable %s has shape %s, the level heights of member 0 %s'
                                 % (i, k, np.shape(m['data'][k]), z0.shape))
        if i == 0:
            continue
        z = np.asarray(m['zlevels'])
        if z.shape != z0.shape:
            raise ValueError('ensemble member %d: z-levels have shape %s, member 0 %s' % (i, z.shape, z0.shape))
        if not np.array_equal(z, z0):
            raise ValueError('ensemble member %d: z-levels differ from member 0 in %d value(s): members share the '
                             'level heights' % (i, int(np.count_nonzero(z != z0))))
        for key in PROJ_KEYS:
            if float(m['proj_info'][key]) != float(ref['proj_info'][key]):
                raise ValueError('ensemble member %d: grid differs from member 0 (proj_info[%r] = %r, not %r)'
                                 % (i, key, m['proj_info'][key], ref['proj_info'][key]))
        if not np.array_equal(np.asarray(m['resolution'], dtype=np.float64),
                              np.asarray(ref['resolution'], dtype=np.float64)):
            raise ValueError('ensemble member %d: grid resolution %r differs from member 0 (%r)'
                             % (i, tuple(m['resolution']), tuple(ref['resolution'])))


def plan_member_chunks(members, bytes_per_member, budget, max_per_chunk=MEMBERS_PER_CALL):
    """Cuts `members` (any sequence) into consecutive chunks for cpol_run_sweep_members: order kept, every member
    exactly once, never an empty chunk, at most `max_per_chunk` members per chunk, and chunk size x bytes_per_member
    <= budget whenever one member fits (a single member that does not fit still gets its chunk of one: the launch
    then reports the shortage itself)."""
    members = list(members)
    per = max(1, int(bytes_per_member))
    n = max(1, min(int(max_per_chunk), int(budget) // per))
    return [members[i:i + n] for i in range(0, len(members), n)]


def choose_form(n_sub, shared_from):
    """form=None: 'shared' (cpol_run_sweep_members) from `shared_from` sub-beams per radial, 'per_member'
    (cpol_select_member + the ordinary sweep, which keeps the fused single-beam kernels) below."""
    return 'shared' if n_sub >= shared_from else 'per_member'
