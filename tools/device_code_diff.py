#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of the library the same, instruction for instruction?  The check behind a change
that touches host code only: it pairs the per-translation-unit code objects of OLD.so and NEW.so (kernel_resources.py
code_objects) by their sets of kernel names, then compares `llvm-objdump -d` per kernel and the `llvm-readelf --notes`
metadata per pair.  A code object whose set of kernels changed (a new signature, a new instantiation) pairs with the one it
shares most names with: the kernels on one side only are named, the shared ones compared.  The __hip_cuid_<hash> symbol
hashes the source text; it is data, in neither.  No GPU needed.

  python tools/device_code_diff.py OLD.so NEW.so      prints the kernels that differ; exit status 1 if any do
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_objects  # noqa: E402


def _tool(name, flag, elf):
    with tempfile.NamedTemporaryFile(suffix='.co') as f:
        f.write(elf)
        f.flush()
        txt = subprocess.run([os.path.join(LLVM, name), flag, f.name], stdout=subprocess.PIPE, check=True).stdout.decode()
    return txt.replace(f.name, '<code object>')


def describe(elf):
    """-> (kernel names, {symbol: its disassembly}, {kernel: its metadata block}, metadata outside the kernel blocks)"""
    code, sym = {}, None
    for line in _tool('llvm-objdump', '-d', elf).splitlines():
        m = re.match(r'[0-9a-f]+ <(.+)>:$', line)
        if m:
            sym = m.group(1)
        if sym:      # without the load address: the symbol's line, and the offset in front of each encoding
            code.setdefault(sym, []).append(re.sub(r'^[0-9a-f]+ <|(?<=// )[0-9A-F]{12}: ', '', line))
    head, *blocks = re.split(r'\n\s*- \.agpr_count:', '\n' + _tool('llvm-readelf', '--notes', elf))
    meta = {}
    for blk in blocks:
        name = re.search(r'\.name:\s*(\S+)', blk)
        # the last kernel's block runs on into the rest of the note (target, version): part of that kernel's text here
        meta[name.group(1) if name else '?'] = blk
    return frozenset(meta), code, meta, head


def diff(old_lib, new_lib, out=sys.stdout):
    old, new = [describe(e) for e in code_objects(old_lib)], [describe(e) for e in code_objects(new_lib)]
    bad, lone = 0, ([], [])
    print('code objects: %d old, %d new' % (len(old), len(new)), file=out)

    def compare(a, b):      # the symbols two code objects share, and their kernels' metadata
        (na, ca, ma, ha), (nb, cb, mb, hb) = a, b
        differ = sorted(k for k in (set(ca) | set(cb)) - (na ^ nb) if ca.get(k) != cb.get(k))
        notes = sorted(k for k in na & nb if ma[k] != mb[k]) + (['(note header)'] if ha != hb else [])
        for k in differ:
            print('DIFFERS   code      %s' % k, file=out)
        for k in notes:
            print('DIFFERS   metadata  %s' % k, file=out)
        print('%-9s %3d kernels, %d symbols: %s ...' % ('same' if not (differ or notes) else 'DIFFERENT', len(na & nb), len(ca), min(na & nb)),
              file=out)
        return len(differ) + len(notes)

    # objects with equal name sets (the host-only translation units have none) pair in link order
    for names in sorted(set(o[0] for o in old) | set(n[0] for n in new), key=lambda s: sorted(s)):
        a, b = [o for o in old if o[0] == names], [n for n in new if n[0] == names]
        if len(a) != len(b):
            lone[0].extend(a)
            lone[1].extend(b)
        elif names:
            bad += sum(compare(x, y) for x, y in zip(a, b))
    # a code object that lost or gained a kernel (a changed signature is both) pairs with the one it shares most names with
    for a in lone[0]:
        b = max(lone[1], key=lambda n: len(n[0] & a[0]), default=None)
        if b is None or not (a[0] & b[0]):
            bad += 1
            print('UNPAIRED  old code object with %d kernels: %s ...' % (len(a[0]), min(a[0])), file=out)
            continue
        lone[1].remove(b)
        for k in sorted(a[0] ^ b[0]):
            bad += 1
            print('%s  %s' % ('ONLY OLD ' if k in a[0] else 'ONLY NEW ', k), file=out)
        bad += compare(a, b)
    for b in lone[1]:
        bad += 1
        print('UNPAIRED  new code object with %d kernels: %s ...' % (len(b[0]), min(b[0])), file=out)
    print('%d difference(s)' % bad, file=out)
    return bad


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(1 if diff(sys.argv[1], sys.argv[2]) else 0)
