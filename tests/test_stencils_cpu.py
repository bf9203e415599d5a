"""Gate stencils without a GPU: the library's set of entry points is what it was (the budget and the report travel through
cpol_debug_read's control names "stencil_budget" and "stencil"), and the header, the library's source and _native.py agree on
those names, on the record's size and on the Python side's keywords."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cosmo_pol_amd', 'csrc')


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_source_and_native_agree_on_the_stencil_names():
    from cosmo_pol_amd import _native as N
    header = _read(ROOT, 'include', 'cosmo_pol_amd.h')
    hip = _read(CSRC, 'cosmo_pol_hip.hip')
    native = _read(ROOT, 'cosmo_pol_amd', '_native.py')
    for name in ('stencil', 'stencil_budget'):
        assert '"%s"' % name in header, name                              # documented with cpol_debug_read
        assert '!strcmp(name, "%s")' % name in hip, name                  # handled
        assert "b'%s'" % name in native, name                             # used by the wrapper
    assert 'stencil' in header[header.index('cpol_mem_info') - 2500:header.index('cpol_mem_info')]      # (its documentation names the store)
    assert callable(N.Context.set_stencil_budget) and callable(N.Context.stencil_state)
    # six figures on both sides
    assert re.search(r'const double v\[6\] = \{\(double\)ctx->last_stencil', hip)
    assert "('form', 'entries', 'bytes', 'records', 'replays', 'drops')" in native
    # the record: 69 bytes per gate, as the views are laid out and as DESIGN.md states
    interp = _read(CSRC, 'cpol_interp.inl')
    assert re.search(r'#define CPOL_STENCIL_BYTES_PER_GATE 69\b', interp)
    steps = [int(x) for x in re.findall(r'b \+= (\d+) \* n;', hip[hip.index('static void stencil_views'):hip.index('// The form of this sweep')])]
    assert sum(steps) + 1 == 69, steps
    assert '69 B' in _read(ROOT, 'DESIGN.md')


def test_no_new_entry_point_and_the_operator_keywords():
    from cosmo_pol_amd import _native as N
    from cosmo_pol_amd import RadarOperator
    assert not any('stencil' in e for e in N.EXPORTS)
    assert 'global: cpol_*;' in _read(CSRC, 'exports.map')
    if os.path.exists(N.LIB_PATH):
        out = subprocess.check_output(['nm', '-D', '--defined-only', N.LIB_PATH]).decode()
        assert 'stencil' not in out
    sig = inspect.signature(RadarOperator.__init__)
    assert sig.parameters['stencil_budget'].default is None and sig.parameters['stencil_budget'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(RadarOperator.stencil_state).parameters) == ['self', 'lane']
