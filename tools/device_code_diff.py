#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of the library the same, instruction for instruction?  The check behind a change
that touches host code only: it pairs the per-translation-unit code objects of OLD.so and NEW.so (kernel_resources.py
code_objects) by their sets of kernel names, then compares `llvm-objdump -d` per kernel and the `llvm-readelf --notes`
metadata per pair.  The __hip_cuid_<hash> symbol hashes the source text; it is data, in neither.  No GPU needed.

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
    bad = 0
    print('code objects: %d old, %d new' % (len(old), len(new)), file=out)
    # objects with equal name sets (the host-only translation units have none) pair in link order
    for names in sorted(set(o[0] for o in old) | set(n[0] for n in new), key=lambda s: sorted(s)):
        a, b = [o for o in old if o[0] == names], [n for n in new if n[0] == names]
        label = min(names) if names else '(no kernels)'
        if len(a) != len(b):
            bad += 1
            print('UNPAIRED  %d old / %d new code objects with these %d kernels: %s ...' % (len(a), len(b), len(names), label), file=out)
            other = set().union(*(s[0] for s in (new if a else old)))      # a lost or gained instantiation is in no set there
            for k in sorted(names - other):
                print('    %s %s' % ('only old:' if a else 'only new:', k), file=out)
            continue
        for (_, ca, ma, ha), (_, cb, mb, hb) in zip(a, b):
            differ = sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))
            notes = sorted(k for k in set(ma) | set(mb) if ma.get(k) != mb.get(k)) + (['(note header)'] if ha != hb else [])
            for k in differ:
                print('DIFFERS   code      %s' % k, file=out)
            for k in notes:
                print('DIFFERS   metadata  %s' % k, file=out)
            bad += len(differ) + len(notes)
            print('%-9s %3d kernels, %d symbols: %s ...' % ('same' if not (differ or notes) else 'DIFFERENT', len(names), len(ca), label),
                  file=out)
    print('%d difference(s)' % bad, file=out)
    return bad


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(1 if diff(sys.argv[1], sys.argv[2]) else 0)
