"""Which product a call carries, or why it is refused (cosmo_pol_amd/csrc/cpol_products.h: call_product) on the host, through
tests/c_host/products_check.cpp: all 2^7 sets of the product pointers of cpol_outputs at each of the four entry points.  No
expected value here comes from call_product: `parent` below walks the pointers the way the entry points and run_sequence did
before the rule moved (cosmo_pol_hip.hip at commit 1be122f, line numbers of that file), and the texts are copied from there:

  cpol_run_columns          the first pointer set is refused, in the order superob, composite, fractions, histogram,
                            spectrum_moments, member_stats, member_verify, ahead of every other argument check     4427-4433
  cpol_run_sweep_members    spectrum_moments is refused behind the basic argument check, ahead of the time blend   4499
  run_sequence              a composite beside superob, histogram, member_stats or spectrum_moments                3113-3116
                            a histogram beside superob, member_stats or spectrum_moments                           3118-3121
                            then block by block: superob (its plan, 3127), orphan member_verify (3134), member_stats (beside
                            superob 3137, in a timed call 3138, its plan 3139), spectrum_moments (beside either 3146, its plan
                            3147), histogram (its plan 3159), composite (its plan 3171), fractions (frac_check without a
                            composite, cpol_frac.h:83, through 3179-3180)

A refusal is due BEFORE any plan when no block in front of it ran a plan, and AFTER the plan of the one block that did: that
plan's own refusals (bad windows, a pass not open, ...) were reported first."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTERS = ('superob', 'member_stats', 'member_verify', 'spectrum_moments', 'histogram', 'composite', 'fractions')
ENTRIES = ('sweep', 'members', 'timed', 'columns')
BOTH = ' are taken by cpol_run_sweep and cpol_run_sweep_members'
COLUMNS = (('superob', 'cpol_run_columns: superobservations (outputs->superob)' + BOTH),
           ('composite', 'cpol_run_columns: gridded composites (outputs->composite)' + BOTH),
           ('fractions', 'cpol_run_columns: neighbourhood verification (outputs->fractions) is taken by cpol_run_sweep and cpol_run_sweep_members'),
           ('histogram', 'cpol_run_columns: sweep histograms (outputs->histogram)' + BOTH),
           ('spectrum_moments', 'cpol_run_columns: spectrum moments (outputs->spectrum_moments) are taken by cpol_run_sweep'),
           ('member_stats', 'cpol_run_columns: ensemble statistics (outputs->member_stats)' + BOTH),
           ('member_verify', 'cpol_run_columns: ensemble verification (outputs->member_verify) is taken by cpol_run_sweep and cpol_run_sweep_members'))
MEMBERS_SM = 'cpol_run_sweep_members: spectrum moments (outputs->spectrum_moments) are taken by cpol_run_sweep'
COMPOSITE = 'cpol_composite: not together with superobservations, histograms, ensemble statistics or spectrum moments in one call'
HISTOGRAM = 'cpol_histogram: not together with superobservations, ensemble statistics or spectrum moments in one call'
VERIFY = 'cpol_member_verify: needs ensemble statistics (outputs->member_stats) in the same call'
STATS_SO = 'cpol_member_stats: not together with superobservations (outputs->superob) in one call'
STATS_TIMED = 'cpol_member_stats: a time-blended call (tables->time_blend) folds no members'
MOMENTS = 'cpol_spectrum_moments: not together with superobservations or ensemble statistics in one call'
FRACTIONS = 'cpol_fractions: needs a composite (outputs->composite) in the same call'


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('products') / 'products_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'cosmo_pol_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'c_host', 'products_check.cpp'), '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def ask(exe, entry, sets):
    r = subprocess.run([exe, entry] + [','.join(s) or '-' for s in sets], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(sets)
    return [tuple(line.split('\t')) for line in lines]


def parent(entry, s):
    """(product, when, text) of the parent commit for the pointer set `s`."""
    if entry == 'columns':
        for name, text in COLUMNS:
            if name in s:
                return 'none', 'entry', text
        return 'none', 'accepted', '-'
    if entry != 'sweep' and 'spectrum_moments' in s:
        return 'none', 'entry', MEMBERS_SM
    planned = []                                               # the blocks whose plan ran: never more than one

    def refused(text):
        return (planned[0], 'after', text) if planned else ('none', 'before', text)
    if 'composite' in s and s & {'superob', 'histogram', 'member_stats', 'spectrum_moments'}:
        return refused(COMPOSITE)
    if 'histogram' in s and s & {'superob', 'member_stats', 'spectrum_moments'}:
        return refused(HISTOGRAM)
    if 'superob' in s:
        planned.append('superob')
    if 'member_verify' in s and 'member_stats' not in s:
        return refused(VERIFY)
    if 'member_stats' in s:
        if 'superob' in s:
            return refused(STATS_SO)
        if entry == 'timed':
            return refused(STATS_TIMED)
        planned.append('member_stats')
    if 'spectrum_moments' in s:
        if s & {'superob', 'member_stats'}:
            return refused(MOMENTS)
        planned.append('spectrum_moments')
    if 'histogram' in s:
        planned.append('histogram')
    if 'composite' in s:
        planned.append('composite')
    if 'fractions' in s and 'composite' not in s:
        return refused(FRACTIONS)
    assert len(planned) <= 1
    return (planned[0] if planned else 'none'), 'accepted', '-'


SETS = [frozenset(c) for n in range(len(POINTERS) + 1) for c in itertools.combinations(POINTERS, n)]


@pytest.mark.parametrize('entry', ENTRIES)
def test_every_pointer_set(exe, entry):
    assert len(SETS) == 128
    got = ask(exe, entry, [sorted(s) for s in SETS])
    for s, g in zip(SETS, got):
        assert g == parent(entry, s), (entry, sorted(s))


def test_written_out(exe):
    # the cases a reader would look up, stated without `parent`
    cases = [
        ('sweep', [], ('none', 'accepted', '-')),
        ('sweep', ['superob'], ('superob', 'accepted', '-')),
        ('members', ['member_stats', 'member_verify'], ('member_stats', 'accepted', '-')),
        ('sweep', ['spectrum_moments'], ('spectrum_moments', 'accepted', '-')),
        ('timed', ['histogram'], ('histogram', 'accepted', '-')),
        ('members', ['composite', 'fractions'], ('composite', 'accepted', '-')),
        # the rows that tests/test_histogram_cpu.py and tests/test_composite_cpu.py held as `other=1`
        ('sweep', ['histogram', 'superob'], ('none', 'before', HISTOGRAM)),
        ('sweep', ['histogram', 'member_stats'], ('none', 'before', HISTOGRAM)),
        ('sweep', ['histogram', 'spectrum_moments'], ('none', 'before', HISTOGRAM)),
        ('sweep', ['composite', 'superob'], ('none', 'before', COMPOSITE)),
        ('sweep', ['composite', 'histogram'], ('none', 'before', COMPOSITE)),
        ('members', ['composite', 'member_stats'], ('none', 'before', COMPOSITE)),
        ('sweep', ['composite', 'spectrum_moments'], ('none', 'before', COMPOSITE)),
        # several faults: the one the parent reported
        ('sweep', ['composite', 'histogram', 'superob', 'fractions'], ('none', 'before', COMPOSITE)),
        ('members', ['composite', 'spectrum_moments'], ('none', 'entry', MEMBERS_SM)),
        ('timed', ['spectrum_moments'], ('none', 'entry', MEMBERS_SM)),
        ('sweep', ['superob', 'member_verify', 'member_stats'], ('superob', 'after', STATS_SO)),
        ('sweep', ['superob', 'member_verify'], ('superob', 'after', VERIFY)),
        ('sweep', ['member_verify', 'composite'], ('none', 'before', VERIFY)),
        ('sweep', ['superob', 'spectrum_moments', 'fractions'], ('superob', 'after', MOMENTS)),
        ('sweep', ['member_stats', 'spectrum_moments'], ('member_stats', 'after', MOMENTS)),
        ('timed', ['member_stats'], ('none', 'before', STATS_TIMED)),
        ('timed', ['superob', 'member_stats'], ('superob', 'after', STATS_SO)),
        ('timed', ['member_stats', 'fractions'], ('none', 'before', STATS_TIMED)),
        ('sweep', ['fractions'], ('none', 'before', FRACTIONS)),
        ('sweep', ['histogram', 'fractions'], ('histogram', 'after', FRACTIONS)),
        ('members', ['member_stats', 'fractions'], ('member_stats', 'after', FRACTIONS)),
        ('columns', [], ('none', 'accepted', '-')),
        ('columns', ['member_verify'], ('none', 'entry', COLUMNS[6][1])),
        ('columns', list(POINTERS), ('none', 'entry', COLUMNS[0][1])),
        ('columns', ['member_stats', 'spectrum_moments', 'histogram'], ('none', 'entry', COLUMNS[3][1])),
    ]
    for entry, s, want in cases:
        assert ask(exe, entry, [s])[0] == want, (entry, s)
