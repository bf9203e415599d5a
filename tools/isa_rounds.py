#!/usr/bin/env python
"""Memory round trips a kernel waits for, counted in cosmo_pol_amd/csrc/cosmo_pol_hip.gfx950.s
(`make -C cosmo_pol_amd/csrc asm`):
    python tools/isa_rounds.py [--asm FILE] [--tag TAG] [name-substring[@split-regex] ...]
For each kernel whose mangled name holds the substring: the instruction count, the s_load count, and the AWAITED
scalar and vector rounds.  A round is an `s_waitcnt` with an lgkmcnt (vmcnt) field that follows at least one s_load /
s_buffer_load (global_ / buffer_ / flat_ / scratch_ load) issued since the previous such wait: loads in flight together
and awaited once are one round, a load awaited alone is a round of its own.  With @regex the counts are also given in
front of and behind the first instruction that matches (k_gate1_ray: the ticket's ds_add_rtn).  The counts are static,
in the order of the text: one path through the kernel executes fewer.  Default kernels: the three of a c2 sweep."""
import argparse
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ['k_gate1_ray8HydroSet@ds_add_rtn', 'k_scan_rays', 'k_interp_replay']
INSTR = re.compile(r'^\s+([a-z]\w+)\b(.*)$')
VLOAD = re.compile(r'^(global|buffer|flat|scratch)_load')
SLOAD = re.compile(r'^s_(buffer_)?load')


def rounds(lines):
    """(instructions, s_loads, scalar rounds, vector rounds) of a stretch of assembly text"""
    n = n_sload = s_rounds = v_rounds = 0
    s_open = v_open = False
    for l in lines:
        m = INSTR.match(l)
        if not m or l.lstrip().startswith(('.', ';')):
            continue
        op, rest = m.group(1), m.group(2)
        n += 1
        if SLOAD.match(op):
            n_sload += 1
            s_open = True
        elif VLOAD.match(op):
            v_open = True
            if op.startswith('flat_'):            # (a flat load counts on both counters)
                s_open = True
        elif op == 's_waitcnt':
            if 'lgkmcnt' in rest and s_open:
                s_rounds += 1
                s_open = False
            if 'vmcnt' in rest and v_open:
                v_rounds += 1
                v_open = False
    return n, n_sload, s_rounds, v_rounds


def kernel_text(s, name):
    i = s.index('\n' + name + ':')
    return s[i:s.index('s_endpgm', i) + 8].split('\n')[2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--asm', default=os.path.join(ROOT, 'cosmo_pol_amd', 'csrc', 'cosmo_pol_hip.gfx950.s'))
    ap.add_argument('--tag', default='')
    ap.add_argument('kernels', nargs='*', default=DEFAULT)
    args = ap.parse_args()
    s = open(args.asm).read()
    names = re.findall(r'^(_Z\w+):', s, flags=re.M)
    print('%-10s %-34s %12s %7s %14s %14s' % ('build', 'kernel', 'instructions', 's_load', 'scalar rounds', 'vector rounds'))
    for spec in args.kernels:
        want, _, split = spec.partition('@')
        for name in [n for n in names if re.search(want, n)]:
            lines = kernel_text(s, name)
            m = re.match(r'_Z(\d+)', name)                      # (_Z<length><name>...: the plain name)
            short = name[m.end():m.end() + int(m.group(1))] if m else name[:34]
            n, nl, sr, vr = rounds(lines)
            extra = ''
            if split:
                at = next((k for k, l in enumerate(lines) if INSTR.match(l) and re.search(split, l)), None)
                if at is not None:
                    b, a = rounds(lines[:at]), rounds(lines[at:])
                    extra = '   in front of %s: %d scalar, %d vector; behind: %d scalar, %d vector' % (split, b[2], b[3], a[2], a[3])
            print('%-10s %-34s %12d %7d %14d %14d%s' % (args.tag, short, n, nl, sr, vr, extra))


if __name__ == '__main__':
    main()
