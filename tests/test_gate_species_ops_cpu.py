"""The host-side filler of k_gate1_ray's species record (cosmo_pol_amd/csrc/cpol_gate_ops.h): every field equals its source for
slots that differ in all of them, the value pointers are vals + var * n, the constants divided on the host have the bits of
classify_item's expressions (compiled without contraction, as the library is), the record is a whole number of 64-byte lines,
and `generic` is set by each excluded case alone and clear for rain, snow and graupel."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_species_record_equals_its_sources(tmp_path):
    exe = str(tmp_path / 'gate_species_ops_check')
    cmd = ['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'c_host', 'gate_species_ops_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'GATE_SPECIES_OPS_OK' in r.stdout, r.stdout + r.stderr
