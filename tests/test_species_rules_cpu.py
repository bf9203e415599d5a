"""What the hydrometeor contributions add to the host-only rules, through tests/c_host/species_check.cpp (its own main):

  cpol_forms.h     FormIn::want_species drops the four single-beam forms (gate1, gate1_species, gate1_ray, fused_gate1) and
                   `graphable`; every other decision is that of the general launch sequence of the same call -- what CPOL_GATE1=0
                   gives it -- and where the plain call takes no single-beam kernel nothing but `graphable` moves at all.  Walked
                   over the FormIn grid of forms_check.cpp under the knobs that reach the single-beam forms.
                   Without the flag choose_forms decides what the parent commit decided: PARENT_DIGEST below is the digest of all
                   60 decisions over that grid, printed by this same program built with -DSPECIES_CHECK_PARENT against the
                   parent commit's cpol_forms.h (which has no such field); the test asks the current header for the same number.
  cpol_buffers.h   BufIn::want_species sizes WB_SZINTEG and moves no other buffer.
  cpol_products.h  `species` alone, with each other product, at each entry point; its refusals stand behind the existing ones."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_DIGEST = '0715565293ff5fe7'          # the parent commit's choose_forms over the 207 360 calls of the walk (see above)
OTHERS = ('superob', 'member_stats', 'member_verify', 'spectrum_moments', 'histogram', 'composite', 'fractions')
TOGETHER = 'cpol_species: not together with another product in one call'
MEMBERS = ('cpol_run_sweep_members: hydrometeor contributions (outputs->species) are taken by cpol_run_sweep and by a time-blended '
           'call, not by the ensemble form')
COLUMNS = ('cpol_run_columns: hydrometeor contributions (outputs->species) are taken by cpol_run_sweep and a time-blended '
           'cpol_run_sweep_members')


def build(tmp, name, flags=()):
    path = str(tmp / name)
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', *flags, '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'c_host', 'species_check.cpp'), '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp('species'), 'species_check')


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_want_species_drops_the_single_beam_forms_and_nothing_else(exe):
    out = run(exe, 'forms')
    assert len(out) == 1 and out[0].startswith('SPECIES_FORMS_OK '), out
    calls, fast = (int(v) for v in out[0].split()[1:])
    assert calls == 8 * 3 * 5 * 3 * 6 * 2 * 4 * 2 * 2 * 3
    assert fast > 1000                      # (the walk does reach calls that give up a single-beam kernel)


def test_without_the_flag_the_forms_are_the_parents(exe):
    out = run(exe, 'digest')
    assert out == ['SPECIES_DIGEST %s %d' % (PARENT_DIGEST, 207360)]


def test_want_species_sizes_the_rows_and_no_other_buffer(exe):
    assert run(exe, 'buffers') == ['SPECIES_BUFFERS_OK 36']


def ask(exe, entry, sets):
    lines = run(exe, 'product', entry, *[','.join(s) or '-' for s in sets])
    assert len(lines) == len(sets)
    return [tuple(line.split('\t')) for line in lines]


def test_species_alone_at_each_entry_point(exe):
    assert ask(exe, 'sweep', [['species']]) == [('species', 'accepted', '-')]
    assert ask(exe, 'timed', [['species']]) == [('species', 'accepted', '-')]
    assert ask(exe, 'members', [['species']]) == [('none', 'before', MEMBERS)]
    assert ask(exe, 'columns', [['species']]) == [('none', 'entry', COLUMNS)]
    assert ask(exe, 'sweep', [[]]) == [('none', 'accepted', '-')]


@pytest.mark.parametrize('entry', ['sweep', 'members', 'timed', 'columns'])
def test_species_with_each_other_product(exe, entry):
    alone = ask(exe, entry, [[o] for o in OTHERS])
    both = ask(exe, entry, [[o, 'species'] for o in OTHERS])
    for o, a, b in zip(OTHERS, alone, both):
        if a[1] != 'accepted':
            assert b == a, (entry, o)       # a call with several faults reports what it always reported
        elif entry == 'members':
            assert b == (a[0], 'after', MEMBERS), (entry, o)
        else:
            assert a[0] != 'none' and b == (a[0], 'after', TOGETHER), (entry, o)


def test_written_out(exe):
    cases = [('sweep', ['species', 'superob'], ('superob', 'after', TOGETHER)),
             ('sweep', ['species', 'composite', 'fractions'], ('composite', 'after', TOGETHER)),
             ('timed', ['species', 'histogram'], ('histogram', 'after', TOGETHER)),
             ('sweep', ['species', 'fractions'], ('none', 'before', 'cpol_fractions: needs a composite (outputs->composite) in the same call')),
             ('sweep', ['species', 'composite', 'histogram'],
              ('none', 'before', 'cpol_composite: not together with superobservations, histograms, ensemble statistics or spectrum moments in one call')),
             ('columns', ['species', 'histogram'],
              ('none', 'entry', 'cpol_run_columns: sweep histograms (outputs->histogram) are taken by cpol_run_sweep and cpol_run_sweep_members')),
             ('members', ['species', 'spectrum_moments'],
              ('none', 'entry', 'cpol_run_sweep_members: spectrum moments (outputs->spectrum_moments) are taken by cpol_run_sweep'))]
    for entry, s, want in cases:
        assert ask(exe, entry, [s])[0] == want, (entry, s)
