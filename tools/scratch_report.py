#!/usr/bin/env python3
"""Where the scratch (spill) accesses of a kernel or of a device function sit.

    make -C speaker-diarization_amd/csrc spkd_hip.gfx950.s
    python tools/scratch_report.py speaker-diarization_amd/csrc/spkd_hip.gfx950.s k_gw
    python tools/scratch_report.py speaker-diarization_amd/csrc/spkd_hip.gfx950.s 'gw_sweep_coarse<1>'
    python tools/scratch_report.py speaker-diarization_amd/csrc/spkd_hip.gfx950.s --frames

NAME is a substring of the symbol; `name<N>` picks the instantiation with the integer
template argument N.  Every symbol that matches is reported: kernels and `noinline` device
functions alike (a function is a symbol of its own in the listing, its scratch is NOT in
the report of the kernel that calls it).  A body runs from the symbol's label to its
`.Lfunc_end` label.  Printed per symbol:

  * lines, DPP instructions, scratch loads / stores, and the `ScratchSize` (bytes per lane),
    VGPRs and occupancy of the metadata behind the body;
  * the save frame: the scratch instructions before the first and after the last
    non-scratch memory instruction.  In a device function the stores at entry and the loads
    at exit are the callee-saved registers of the calling convention, written and read back
    once per CALL whatever the function does in between;
  * for every backward branch (a loop) the number of scratch instructions inside it.  The
    loop that contains the elimination code (the DPP instructions) is the item loop.

--frames lists every device function of the listing that has a save frame."""
import re
import sys

MEM = re.compile(r'^\s*((global|flat|buffer|ds)_|s_(buffer_)?load)')
META = (('scratch', r'; ScratchSize: (\d+)'), ('vgprs', r'; NumVgprs: (\d+)'), ('occupancy', r'; Occupancy: (\d+)'))


def symbols(lines):
    """[(symbol, is_kernel, first body line, end-label line, metadata dict)] in listing order."""
    out = []
    types = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r'\s*\.type\s+(\S+),@function', l)] if m]
    for n, (i, sym) in enumerate(types):
        stop = types[n + 1][0] if n + 1 < len(types) else len(lines)
        start = next((k for k in range(i, stop) if lines[k].startswith(sym + ':')), None)
        end = next((k for k in range(i, stop) if re.match(r'\.Lfunc_end\d+:', lines[k])), None)
        if start is None or end is None:
            continue
        meta, kernel = {}, False
        for k in range(end, stop):
            kernel = kernel or lines[k].startswith('; Kernel info:')
            for key, pat in META:
                m = re.match(pat, lines[k])
                if m:
                    meta[key] = int(m.group(1))
        out.append((sym, kernel, start + 1, end, meta))
    return out


def frame(body):
    """(stores, loads) among the scratch instructions before the first non-scratch memory
    instruction, and the same after the last one."""
    mem = [i for i, l in enumerate(body) if MEM.match(l)]
    first, last = (mem[0], mem[-1]) if mem else (len(body), -1)
    count = lambda part: (sum('scratch_store' in l for l in part), sum('scratch_load' in l for l in part))
    return count(body[:first]), count(body[last + 1:])


def pretty(sym):
    """spkd::name<N> out of the mangled symbol, where it has that form."""
    m = re.match(r'_ZN4spkdL?(\d+)', sym)
    if not m:
        return sym
    name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
    t = re.match(r'ILi(\d+)EE', rest)
    return name + ('<%s>' % t.group(1) if t else '')


def report(lines, sym, kernel, start, end, meta):
    body = [l.split(';')[0] for l in lines[start:end]]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r'^(\.LBB\d+_\d+):', l)] if m}
    dpp = [i for i, l in enumerate(body) if 'row_newbcast' in l]
    sload = [i for i, l in enumerate(body) if 'scratch_load' in l]
    sstore = [i for i, l in enumerate(body) if 'scratch_store' in l]
    print('%s (%s): %d lines, %d DPP, %d scratch loads, %d scratch stores' % (
        pretty(sym), 'kernel' if kernel else 'device function', len(body), len(dpp), len(sload), len(sstore)))
    print('  ScratchSize %s B per lane, %s VGPRs%s' % (
        meta.get('scratch', '?'), meta.get('vgprs', '?'),
        ', occupancy %d' % meta['occupancy'] if 'occupancy' in meta else ''))
    (es, el), (xs, xl) = frame(body)
    print('  before the first non-scratch memory instruction: %d scratch stores, %d loads; after the last: %d stores, %d loads%s' % (
        es, el, xs, xl, '  <- save frame' if not kernel and (es or xl) else ''))
    loops = []
    for i, l in enumerate(body):
        m = re.search(r's_c?branch\w* (\.LBB\d+_\d+)', l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    for lo, hi in sorted(set(loops)):
        nd = sum(1 for k in dpp if lo <= k <= hi)
        nl = sum(1 for k in sload if lo <= k <= hi)
        ns = sum(1 for k in sstore if lo <= k <= hi)
        if hi - lo > 200 or nl or ns:
            print('  loop lines %6d..%6d (%5d instr): %5d DPP, %4d scratch loads, %4d scratch stores' % (lo, hi, hi - lo, nd, nl, ns))


def frames(lines):
    """Every device function with a save frame; returns their number."""
    n = 0
    for sym, kernel, start, end, meta in symbols(lines):
        if kernel:
            continue
        (es, _), (_, xl) = frame([l.split(';')[0] for l in lines[start:end]])
        if es or xl:
            n += 1
            print('%-24s %4d scratch stores at entry, %4d loads at exit, ScratchSize %s B per lane' % (
                pretty(sym), es, xl, meta.get('scratch', '?')))
    print('%d device function(s) with a save frame' % n)
    return n


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    path, name = sys.argv[1], sys.argv[2]
    lines = open(path).read().splitlines()
    if name == '--frames':
        frames(lines)
        return
    m = re.match(r'^(\w+)<(\d+)>$', name)
    want = re.compile(re.escape(m.group(1)) + 'ILi' + m.group(2) + 'E' if m else re.escape(name))
    found = [s for s in symbols(lines) if want.search(s[0])]
    if not found:
        sys.exit('no kernel or device function matches %s' % name)
    for s in found:
        report(lines, *s)


if __name__ == '__main__':
    main()
