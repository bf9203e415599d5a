#!/usr/bin/env python
"""Where a wavefront of k_gate1_ray spends its time (library built with -DCPOL_SUBSUM_TRACE):
   tools/variants.sh "g1trace|-DCPOL_SUBSUM_TRACE||python tools/gate1_trace.py"
Every wavefront (gate tile, ray, species) records the 100-MHz clock at: entry (in front of the workgroup barrier), barrier
passed, presence words arrived, model values arrived, PSD parameters done, gather + Horner done, terms in LDS + ticket taken,
and -- the wavefront that finishes the tile -- gates finished.  A wavefront that returns behind the presence test (its
species absent from the tile) records entry, barrier, presence and the moment it leaves; its life is entry -> leaving.
Round 10: inside the PSD parameters the moment the species' rule is done (its scalar operands have all arrived, the slope is
formed: `us_rule`, the rest of `us_parameters` is the table position and the fall-speed moments), and the finish in parts,
each the latest lane's, counted from the ticket: the species' sums read from LDS, the polarimetric part done and its eight
stores issued, RVEL's operands arrived (the projection known), arithmetic done (RVEL and mask formed), stores issued; what
is left of the finish is the wait for the stores.
Round 11: model values arrived -> the first coefficient rows requested (`us_first_request`, the latest lane's; beside `us_rule`).
A wavefront whose slot takes the compact species record forms its scale and moments behind that request, inside the gather:
its `us_parameters` ends with the position on the panel axis.  A build without the point (bits 20-31 of word 6 zero
everywhere) reports None: there the request follows the parameters, `us_parameters` is its figure.
ONE isolated c2 sweep on one lane (CPOL_GATE1_RAY=1), and one of three lanes in flight."""
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('CPOL_GATE1_RAY', '1')
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from cosmo_pol_amd import RadarOperator  # noqa: E402


def report(tag, tr):
    used = tr[:, 0] > 0
    t = tr[used].astype(np.int64)
    nv = (tr[used, 6] & np.uint64(0xFF)).astype(np.int64)
    t_rule = ((tr[used, 6] >> np.uint64(8)) & np.uint64(0xFFF)).astype(np.int64)        # values arrived -> the species' rule done
    t_req = ((tr[used, 6] >> np.uint64(20)) & np.uint64(0xFFF)).astype(np.int64)        # values arrived -> first coefficient rows requested
    sp = ((tr[used, 6] >> np.uint64(32)) & np.uint64(0xFF)).astype(np.int64)
    t_bar = ((tr[used, 6] >> np.uint64(40)) & np.uint64(0xFFF)).astype(np.int64)      # entry -> barrier passed
    t_pre = ((tr[used, 6] >> np.uint64(52)) & np.uint64(0xFFF)).astype(np.int64)      # entry -> presence words known
    base = t[:, 0].min()
    us = lambda a: a / 100.0
    ph = np.stack([np.maximum(t[:, 1] - t[:, 0] - t_pre, 0), t[:, 2] - t[:, 1], t[:, 3] - t[:, 2], t[:, 4] - t[:, 3]], axis=1)
    last = t[:, 5] > 0
    fin = np.where(last, t[:, 5] - t[:, 4], 0)
    life = np.where(last, t[:, 5], t[:, 4]) - t[:, 0]
    heavy = nv > 0
    out = {'tag': tag, 'wavefronts': int(used.sum()), 'with_items': int(heavy.sum()),
           'span_us': round(us(np.where(last, t[:, 5], t[:, 4]).max() - base), 1),
           'all_started_after_us': round(us(t[:, 0].max() - base), 1)}
    for name, m in (('with_items', heavy), ('empty', ~heavy)):
        if m.any():
            out[name] = {'n': int(m.sum()), 'mean_valid_lanes': round(float(nv[m].mean()), 1),
                         'us_barrier': round(float(us(t_bar[m]).mean()), 2), 'us_presence': round(float(us(t_pre[m] - t_bar[m]).mean()), 2),
                         'finishers': int((m & last).sum()),
                         'us_life_not_finishing': round(float(us(life[m & ~last]).mean()), 2) if (m & ~last).any() else None,
                         'us_values': round(float(us(ph[m, 0]).mean()), 2), 'us_parameters': round(float(us(ph[m, 1]).mean()), 2),
                         'us_rule': round(float(us(t_rule[m]).mean()), 2),
                         'us_first_request': round(float(us(t_req[m & (t_req > 0)]).mean()), 2) if (m & (t_req > 0)).any() else None,
                         'us_gather_horner': round(float(us(ph[m, 2]).mean()), 2), 'us_lds_ticket': round(float(us(ph[m, 3]).mean()), 2),
                         'us_life_mean': round(float(us(life[m]).mean()), 2), 'us_life_p95': round(float(np.percentile(us(life[m]), 95)), 2)}
    if last.any():
        out['finishing'] = {'n': int(last.sum()), 'us_finish_mean': round(float(us(fin[last]).mean()), 2)}
        w7 = tr[used, 7][last]
        parts = (w7 & np.uint64(0xFFFFFFFF)) | ((w7 >> np.uint64(36)) << np.uint64(32))
        cum = np.stack([((parts >> np.uint64(12 * q)) & np.uint64(0xFFF)).astype(np.int64) for q in range(5)], axis=1)
        full = (cum > 0).all(axis=1)                          # (a tile without RVEL or without a gate to finish has no parts)
        if full.any():
            c = cum[full]
            names = ('us_sums_read', 'us_pol_done', 'us_operands_arrived', 'us_arithmetic_done', 'us_stores_issued')
            out['finishing'].update({'n_parts': int(full.sum()), 'since_ticket': {k: round(float(us(c[:, q]).mean()), 2) for q, k in enumerate(names)},
                                     'us_entry_to_operands': round(float(us(c[:, 2]).mean()), 2),
                                     'us_operand_wait': round(float(us(c[:, 2] - c[:, 1]).mean()), 2),
                                     'us_store_wait': round(float(us(fin[last][full] - c[:, 4]).mean()), 2)})
    out['by_species_us_life'] = {int(k): round(float(us(life[(sp == k) & heavy]).mean()), 2) for k in np.unique(sp) if ((sp == k) & heavy).any()}
    # per gate tile (blockIdx.x = the workgroup's linear index mod 8): how much work it holds, when its last wavefront ends, and
    # on which XCD (XCC_ID of the hardware register) its wavefronts ran
    idx = np.nonzero(used)[0]
    tile = (idx // 3) % 8
    end = np.where(last, t[:, 5], t[:, 4])
    xcc = ((tr[used, 7] >> np.uint64(32)) & np.uint64(15)).astype(np.int64)
    out['by_tile'] = {int(k): {'with_items': int((heavy & (tile == k)).sum()), 'wave_us': round(float(us(life[tile == k]).sum()), 0),
                               'last_end_us': round(float(us(end[tile == k].max() - base)), 1),
                               'xcc_ids': sorted(set(xcc[tile == k].tolist()))} for k in range(8)}
    print(json.dumps(out), flush=True)


def main():
    conf, hyds, cube, luts = bench.make_inputs('c2', False)
    with contextlib.redirect_stdout(sys.stderr):
        op = RadarOperator(config=conf, luts=luts, output_variables='only_radar')
        op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    lanes = [op._lane(i) for i in range(3)]
    az = np.arange(0, 360, 1.0)
    els = [np.full(360, e) for e in bench.C2_ELEVATIONS[:8]]
    ng = len(op.constants.RANGE_RADAR)
    slabs = [torch.empty((9, 360, ng), dtype=torch.float32, device='cuda') for _ in range(3)]
    outs = [{k: s[i].data_ptr() for i, k in enumerate(bench.RADAR_FIELDS)} for s in slabs]
    N = 131072
    for _ in range(4):
        op.simulate_rays(az, els[0], device_outputs=outs[0], lane=0)
    op.wait(0)
    torch.cuda.synchronize()
    report('isolated sweep', op._ctx.debug_read('subsum_trace', (N, 8), np.uint64))
    for k in range(48):
        op.simulate_rays(az, els[k % 8], device_outputs=outs[k % 3], lane=k % 3)
    for i in range(3):
        op.wait(i)
    torch.cuda.synchronize()
    report('a sweep among three lanes in flight (the last writer of every slot)', op._ctx.debug_read('subsum_trace', (N, 8), np.uint64))
    op.close()


if __name__ == '__main__':
    main()
