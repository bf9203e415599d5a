"""Worker of tests/test_gpu_terrain_shadow.py::test_sharded_volume_under_shadowing: RadarOperator(distributed=True).get_PPI with
terrain shadowing and the visibility on, the rays of every sweep sharded over the ranks, against the same scan computed by each
rank alone, bit for bit -- `visibility` among the gathered fields.  CPOL_DIST_BACKEND=nccl: one rank per GPU over RCCL; the
default (gloo) puts every rank on GPU 0, as tests/_dist_gpu_worker.py does."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    backend = os.environ.get('CPOL_DIST_BACKEND', 'gloo')
    local = int(os.environ.get('LOCAL_RANK', '0')) if backend == 'nccl' else 0
    if backend == 'nccl':
        import torch
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    else:
        dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    import test_gpu_terrain_shadow as T
    from cosmo_pol_amd import RadarOperator
    conf, luts, cube = T.config_for('3x3', T.ON)
    azs = np.array([30.0, 60.0, 75.0, 90.0, 105.0, 120.0, 150.0])       # 7 rays: an uneven split
    scans = []
    for distributed in (True, False):
        op = RadarOperator(config=conf, luts=luts, output_variables='only_radar', device=local, distributed=distributed)
        op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
        scans.append(op.get_PPI(elevations=[1.0, 3.0], azimuths=azs))
        op.close()
    a, b = scans
    assert 'visibility' in a.fields and 'visibility' in b.fields
    for k in b.fields:
        if k not in a.fields:
            continue
        x, y = np.ma.asarray(a.fields[k]['data']), np.ma.asarray(b.fields[k]['data'])
        assert x.shape == y.shape, k
        assert np.array_equal(np.ma.getmaskarray(x), np.ma.getmaskarray(y)), k
        assert np.array_equal(x.filled(0), y.filled(0)), (k, rank)
    vis = np.ma.asarray(b.fields['visibility']['data']).filled(np.nan)
    assert (vis == 0.0).any() and (vis == 1.0).any() and ((vis > 0) & (vis < 1)).any()
    dist.barrier()
    if rank == 0:
        print('SHADOW_DIST_OK world=%d backend=%s fields=%d' % (world, backend, len(a.fields)))
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
