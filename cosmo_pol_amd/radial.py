"""Radial records over the batched results of the HIP path.

The reference hands lists of `Radial` objects from the scan loop to
`cut_at_sensitivity` and `PyartRadop` (cosmo_pol/interpolation/radial.py:17-54,
cosmo_pol/radar_operator.py:411-421, 445-451).  The HIP path returns one
[n_rays, n_gates] array per variable; `to_radials` re-expresses such a result as
the reference's per-radial records (row views, no copies), so reference-side code
that consumes lists of radials -- `cut_at_sensitivity(list_sweeps)`,
`PyartRadop('ppi', {... 'data': list_sweeps})` -- runs on it unchanged
(level B).
"""
import numpy as np

# keys of a simulate_rays result that are not simulated / model variables
_GEOMETRY = ('mask', 'lats', 'lons', 'dist', 'heights', 'n_sub', 'model_vars')


class Radial(object):
    """Same attributes as cosmo_pol.interpolation.radial.Radial (radial.py:17-54)."""

    def __init__(self, dic_values, mask, lats_profile, lons_profile, dist_ground_profile,
                 heights_profile, elev_profile=None, quad_pt=None, quad_weight=1):
        self.mask = mask
        self.quad_pt = [] if quad_pt is None else quad_pt
        self.quad_weight = quad_weight
        self.lats_profile = lats_profile
        self.lons_profile = lons_profile
        self.dist_profile = dist_ground_profile
        self.heights_profile = heights_profile
        self.elev_profile = [] if elev_profile is None else elev_profile
        self.values = dic_values
        # only meaningful for sub-radials inside the melting scheme (radial.py:50-53)
        self.has_melting = False
        self.mask_ml = None


def to_radials(result, azimuths=None, elevations=None, model_names=None):
    """`result`: dict of [n_rays, n_gates] arrays as returned by
    RadarOperator.simulate_rays (or one packaged sweep of RadarScan.raw, whose variables sit
    under 'fields').  Returns one Radial per ray whose `values` are row VIEWS of the batched
    arrays (so censoring them in place, as cut_at_sensitivity does, edits the batch).
    `azimuths` / `elevations` fill `quad_pt` = [azimuth, elevation] of the integrated radial's
    central sub-beam when given (doppler_scatter.py:480-489 leaves it empty)."""
    if 'fields' in result:                                  # a packaged sweep
        variables = dict(result['fields'])
        azimuths = result.get('azimuth') if azimuths is None else azimuths
        elevations = result.get('elevation') if elevations is None else elevations
    else:
        variables = {k: v for k, v in result.items() if k not in _GEOMETRY}
        if 'model_vars' in result and model_names is not None:
            for i, name in enumerate(model_names):
                variables[name] = result['model_vars'][i]
    n_rays = np.asarray(result['mask']).shape[0]
    out = []
    for r in range(n_rays):
        values = {k: v[r] for k, v in variables.items()}
        qp = []
        if azimuths is not None and elevations is not None:
            qp = [float(np.asarray(azimuths).reshape(-1)[r]), float(np.asarray(elevations).reshape(-1)[r])]
        out.append(Radial(values, result['mask'][r], result['lats'][r], result['lons'][r],
                          result['dist'][r], result['heights'][r], quad_pt=qp))
    return out


def _nansum_pair(x, y):
    """nansum_arr of the reference (utilities.py:231-261) for equal shapes or a length-1 seed: NaN counts as 0."""
    x = np.array(x)
    y = np.array(y)
    if x.shape != y.shape:
        x = np.pad(x, [(0, max(0, d2 - d1)) for d1, d2 in zip(x.shape, y.shape)], 'constant', constant_values=0)
        y = np.pad(y, [(0, max(0, d1 - d2)) for d1, d2 in zip(x.shape, y.shape)], 'constant', constant_values=0)
    return np.nansum([x, y], axis=0)


def integrate_radials(list_subradials):
    """The reference's integrate_radials (interpolation/interpolation.py:36-89) on host NumPy: the model variables of
    the sub-radials averaged with their quadrature weights (NaN skipped), the mask averaged over the sub-radials with
    values in (-1, 0] set to 0, and the central sub-radial's geometry (index int(n / 2)).  Any object with the
    attributes of the reference's Radial is accepted; the records are not modified."""
    n = len(list_subradials)
    if n == 0:
        raise ValueError('integrate_radials: empty list of sub-radials')
    sum_w = 0
    for sb in list_subradials:
        sum_w = sum_w + sb.quad_weight
    values = {}
    for k in list_subradials[0].values.keys():
        acc = np.array([np.nan])
        for sb in list_subradials:
            acc = _nansum_pair(acc, sb.values[k] * sb.quad_weight / sum_w)
        values[k] = acc
    mask = np.zeros(len(list_subradials[0].mask))
    for sb in list_subradials:
        mask = mask + sb.mask
    mask /= float(n)
    mask[np.logical_and(mask > -1, mask <= 0)] = 0
    c = list_subradials[int(n / 2)]
    return Radial(values, mask, c.lats_profile, c.lons_profile, c.dist_profile, c.heights_profile)


def combine_subradials(list_of_subradials):
    """The reference's combine_subradials (utilities/utilities.py:263-283): the variables of radials on the same
    range gates merged into the first one (in place, as there); None, with a notice, when the distances differ."""
    x = list_of_subradials[0]
    for r in list_of_subradials:
        if np.array_equal(np.asarray(r.dist_profile), np.asarray(x.dist_profile)):
            x.values.update(r.values)
        else:
            print('Beams are not defined on the same set of coordinates, aborting')
            return None
    return x


def subradials_to_columns(list_subradials, names, with_melting):
    """The sub-radials of ONE radial (objects with the attributes of the reference's Radial) -> the columns dict of
    RadarOperator.simulate_columns with n_rays = 1.  The records are read, never modified.  ValueError for an empty or
    ragged list (different gate counts: the reference pads those only for its GPM path), a missing variable, or scalar
    and per-gate weights mixed.  `with_melting`: records that carry QmS_v hand their melting fields on as given."""
    subs = list(list_subradials)
    if not subs:
        raise ValueError('empty list of sub-radials')
    n_sub = len(subs)
    n_gates = len(np.asarray(subs[0].mask))
    for sb in subs:
        if len(np.asarray(sb.mask)) != n_gates or len(np.asarray(sb.elev_profile)) != n_gates or \
                any(len(np.asarray(sb.values[k])) != n_gates for k in names if k in sb.values):
            raise ValueError('sub-radials of different lengths are not supported')
    cols = {}
    for k in names:
        if any(k not in sb.values for sb in subs):
            raise ValueError('the sub-radials lack the variable %s' % k)
        cols[k] = np.stack([np.asarray(sb.values[k], dtype=np.float32) for sb in subs])[None]
    cols['elev'] = np.stack([np.asarray(sb.elev_profile, dtype=np.float32) for sb in subs])[None]
    cols['mask'] = np.stack([np.asarray(sb.mask) for sb in subs]).astype(np.int8)[None]
    cols['quad_pts'] = np.asarray([[sb.quad_pt[0], sb.quad_pt[1]] for sb in subs], dtype=np.float64)[None]
    scalar = [np.ndim(sb.quad_weight) == 0 for sb in subs]
    if all(scalar):
        cols['quad_weights'] = np.asarray([float(sb.quad_weight) for sb in subs])
    elif not any(scalar):
        w = [np.asarray(sb.quad_weight, dtype=np.float64) for sb in subs]
        if any(x.shape != (n_gates,) for x in w):
            raise ValueError('per-gate weights must hold one value per gate')
        cols['quad_weights'] = np.stack(w)[None]
    else:
        raise ValueError('scalar and per-gate weights mixed in one radial')
    for k in ('lats_profile', 'lons_profile', 'dist_profile', 'heights_profile'):
        if all(getattr(sb, k, None) is not None for sb in subs):
            cols[k[:-8] if k != 'dist_profile' else 'dist'] = np.stack([np.asarray(getattr(sb, k)) for sb in subs])[None]
    if with_melting and all('QmS_v' in sb.values for sb in subs):
        for k, dt in (('QmS_v', np.float32), ('QmG_v', np.float32), ('fwet_mS', np.float64), ('fwet_mG', np.float64)):
            cols[k] = np.stack([np.asarray(sb.values[k], dtype=dt) for sb in subs])[None]
        cols['has_melting'] = np.asarray([[bool(getattr(sb, 'has_melting', True)) for sb in subs]], dtype=np.int8)
    return cols
