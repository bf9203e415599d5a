"""Terrain shadowing: a sub-beam stays blocked behind its first gate below the topography -- the rule in NumPy.

The library does this on the GPU (k_terrain_shadow, k_visibility: csrc/cpol_shadow.inl); include/cosmo_pol_amd.h states the
same text.  Replaces in the reference: nothing that runs -- interpolation_c.c:92-102 means to fill every gate from the hit onward
("We hit a mountain"), but its own loop overwrites those gates, so that every gate depends on itself alone.  That stays the
default; `integration/terrain_shadow: 1` turns the persistence along range on.

A ROW is one sub-beam of one ray: the last axis of every array here.  Its codes c[g] are as the interpolation leaves them: 0 valid,
+1 above the model top, -1 below the topography or variable 0 NaN (2: outside the domain).

    first = min{ g : c[g] == -1 }, or n_gates when there is none
    for every g >= first: c[g] = -1 and every model variable of that sub-beam gate becomes NaN (a +1 behind the hit becomes -1)
    gates g < first keep their bits; lats, lons, dist, heights, elev are never touched

The step runs after the interpolation and before melting, the 'ml' weights, the classification and everything behind them.

VISIBILITY per ray and gate, float64: S = +0.0; for s ascending S += w[s] where c[r, s, g] != -1; visibility = S / W with W the sum
of w[s] ascending from +0.0.  Exactly 1.0 where no sub-beam is blocked, exactly 0.0 where all are.  Not defined with per-gate
weights (integration scheme 'ml')."""
import numpy as np

# the keys of an interpolate_rays dict that are no model variables: never touched
GEOMETRY = ('lats', 'lons', 'dist', 'heights', 'elev')
_NOT_VALUES = GEOMETRY + ('mask', 'quad_pts', 'quad_weights', 'QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG', 'mask_ml', 'has_melting')


def hit(mask):
    """True from the first code -1 of every row onward."""
    return np.maximum.accumulate(np.asarray(mask) == -1, axis=-1)


def first_hit(mask):
    """Index of the first code -1 of every row (the last axis), n_gates where there is none."""
    mask = np.asarray(mask)
    below = mask == -1
    return np.where(below.any(axis=-1), below.argmax(axis=-1), mask.shape[-1])


def apply_arrays(mask, vals):
    """mask [..., n_gates] codes, vals [n_vars, ..., n_gates] float32 -> their shadowed copies."""
    mask = np.array(mask, dtype=np.int8)
    vals = np.array(vals, dtype=np.float32)
    h = hit(mask)
    mask[h] = -1
    vals[:, h] = np.float32(np.nan)
    return mask, vals


def apply(columns):
    """The dict of RadarOperator.interpolate_rays(melting=False) -> a shadowed copy: the codes and every model variable by the
    rule above, everything else (geometry, quadrature points and weights) as it came.  Columns that carry melting fields are
    refused: the step belongs in front of the melting scheme."""
    if 'mask' not in columns:
        raise ValueError("shadow.apply: the columns carry no 'mask'")
    given = [k for k in ('QmS_v', 'QmG_v', 'fwet_mS', 'fwet_mG', 'mask_ml') if k in columns]
    if given:
        raise ValueError('shadow.apply: columns with melting fields %s: shadow the columns of interpolate_rays(melting=False)' % given)
    mask = np.array(columns['mask'], dtype=np.int8)
    h = hit(mask)
    out = dict(columns)
    mask[h] = -1
    out['mask'] = mask
    for k, a in columns.items():
        if k in _NOT_VALUES:
            continue
        a = np.array(a)
        if a.shape != mask.shape:
            raise ValueError('shadow.apply: %s has shape %s, the mask %s' % (k, a.shape, mask.shape))
        a[h] = np.nan
        out[k] = a
    return out


def visibility(mask, weights):
    """mask [n_rays, n_sub, n_gates] codes, weights [n_sub] -> the visible share of the antenna pattern [n_rays, n_gates] float64."""
    mask = np.asarray(mask)
    w = np.asarray(weights, dtype=np.float64)
    if mask.ndim != 3 or w.shape != (mask.shape[1],):
        raise ValueError("shadow.visibility: mask [n_rays, n_sub, n_gates] and one weight per sub-beam (not defined with the "
                         "per-gate weights of integration scheme 'ml')")
    s_w = np.zeros((mask.shape[0], mask.shape[2]), dtype=np.float64)
    total = np.float64(0.0)
    for s in range(mask.shape[1]):
        seen = mask[:, s, :] != -1
        s_w[seen] = s_w[seen] + w[s]
        total = total + w[s]
    return s_w / total
