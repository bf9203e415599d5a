"""k_gate1_ray's workgroup -> (rays x gates) tile decode (cosmo_pol_amd/csrc/cpol_tile.h) on the host: every gate of
the sweep exactly once, every 32-gate segment of a row (and every 128-B line of an output whose rows are a multiple of
128 B) from one XCD class, the XCD classes evenly loaded -- for every tile shape the build knob allows and for sweep
shapes that are not multiples of the tile."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(360, 500), (359, 497), (17, 3), (1, 1), (1, 500), (360, 1), (2, 33), (64, 64), (225, 500), (1800, 125), (100, 96), (17, 32), (359, 512)]


@pytest.mark.parametrize('tg', range(7))
def test_gate1_tile_decode_is_a_bijection_with_lines_on_one_xcd(tmp_path, tg):
    exe = str(tmp_path / 'gate_tiles_check')
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-DCPOL_GATE1_TILE_GATES_LOG2=%d' % tg,
           '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'c_host', 'gate_tiles_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [str(v) for s in SHAPES for v in s]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'GATE_TILES_OK' in r.stdout, r.stdout + r.stderr
