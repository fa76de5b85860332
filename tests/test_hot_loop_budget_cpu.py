"""Static instruction budget of the headline kernel's hot loops, read from the code objects inside the built library
(no GPU).  welch4096ws is VALU-issue bound: its time follows the number of instructions a segment costs, so
the counts the source was shaped for are pinned here against a compiler or source change that silently brings them back.

A loop is a backward branch and the instructions it spans.  Of the loops that hold an s_barrier (one per segment step):
  * the producer's hot loop is the innermost one that issues exactly eight sample loads (global_load_dwordx2) per barrier -
    the straight-line (false, mid) flavour of item() - and that no branch outside it enters except at its head (the
    chunk walk around it is laid out as backward branches with side entries); it may hold one or two segments per trip,
    so its counts are divided by its barrier count;
  * the consumer's loops are those without any vector-memory instruction; the largest is its main loop, the smaller ones
    the idle-step loop inside it, whose instructions are not part of a segment's path and are taken out of the count.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

VMEM = ('global_', 'buffer_', 'flat_', 'scratch_')


def _kernels():
    import isa_async_hazard
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    out = {}
    for name, ins, labels in isa_async_hazard.objdump_kernels(_hip.LIB_PATH, skip_objects_with=(b'any_fft_kernel',)):
        if 'welch4096ws' in name:
            out[name] = (ins, labels)
    return out


def _loops(ins, labels):
    """-> [(first, last)] of every backward branch that spans an s_barrier"""
    out = []
    for i, (op, args, _) in enumerate(ins):
        if op.startswith('s_cbranch') or op == 's_branch':
            t = labels.get(args.strip())
            if t is not None and t <= i and any(ins[k][0] == 's_barrier' for k in range(t, i + 1)):
                out.append((t, i))
    return out


def _count(ins, idx):
    ops = [ins[k] for k in idx]
    return dict(valu=sum(o.startswith('v_') for o, _, _ in ops),
                vmcnt=sum(o == 's_waitcnt' and 'vmcnt' in a for o, a, _ in ops),
                scratch=sum(o.startswith('scratch_') for o, _, _ in ops),
                barriers=sum(o == 's_barrier' for o, _, _ in ops),
                loads=sum(o.startswith('global_load_dwordx2') for o, _, _ in ops),
                nop=sum(o == 's_nop' for o, _, _ in ops))


def hot_loops(ins, labels):
    """-> (producer hot loop counts, consumer segment-path counts)"""
    loops = _loops(ins, labels)
    assert loops
    innermost = [l for l in loops if not any(m != l and l[0] <= m[0] and m[1] <= l[1] for m in loops)]
    def closed(a, b):
        return not any((op.startswith('s_cbranch') or op == 's_branch') and a < labels.get(args.strip(), -1) <= b
                       for k, (op, args, _) in enumerate(ins) if not a <= k <= b)
    prod = [c for c in (_count(ins, range(a, b + 1)) for a, b in innermost if closed(a, b))
            if c['loads'] and c['loads'] == 8 * c['barriers']]
    assert len(prod) == 1, prod
    cons = [l for l in loops if not any(ins[k][0].startswith(VMEM) for k in range(l[0], l[1] + 1))]
    assert cons
    main = max(cons, key=lambda l: l[1] - l[0])
    idle = set()
    for l in cons:
        if l != main:
            idle.update(range(l[0], l[1] + 1))
    path = _count(ins, [k for k in range(main[0], main[1] + 1) if k not in idle])
    whole = _count(ins, sorted(set(range(main[0], main[1] + 1)) | idle))
    path['vmcnt'], path['scratch'] = whole['vmcnt'], whole['scratch']      # nothing of the kind anywhere in the consumer's loops
    return prod[0], path


def _find(ks, kernel, flags):
    names = [n for n in ks if re.search(r'\d+%sI%sE' % (kernel, ''.join('Lb%dE' % f for f in flags)), n)]
    assert len(names) == 1, (kernel, flags, sorted(ks))
    return ks[names[0]]


def test_welch4096ws_hot_loop_instruction_budget():
    """welch4096ws_compl_kernel<true, true> is what the flagship plan (periodic Hann, constant detrend) launches.  Producer:
    at most 299 VALU instructions per segment (311 in the general build: nine stored pass-1 twiddle powers bring twelve
    fewer, thirteen stored - what ships - twenty-eight, and the chain of sample sums starts without its 0 + r).  Consumer:
    at most 407 per segment, and no s_waitcnt vmcnt inside its loops (fifteen in front of the pass-2 twiddle products
    before the table loads were waited for once, in front of the loop).  No scratch access in either.  The general build
    is held to what it had - 311 and 407 - and to the same absence of waits, since both share the consumer."""
    ks = _kernels()
    prod, cons = hot_loops(*_find(ks, 'welch4096ws_compl_kernel', (1, 1)))
    print('complementary build: producer %s, consumer %s' % (prod, cons))
    assert prod['valu'] <= 299 * prod['barriers'], prod
    assert prod['scratch'] == 0
    assert 300 <= cons['valu'] <= 407, cons
    assert cons['vmcnt'] == 0 and cons['scratch'] == 0, cons
    gprod, gcons = hot_loops(*_find(ks, 'welch4096ws_kernel', (1, 1)))
    print('general build: producer %s, consumer %s' % (gprod, gcons))
    assert gprod['valu'] <= 311 * gprod['barriers'] and gprod['scratch'] == 0, gprod
    assert 300 <= gcons['valu'] <= 407 and gcons['vmcnt'] == 0 and gcons['scratch'] == 0, gcons


def test_welch4096ws_complementary_builds_fit_two_workgroups_per_cu():
    """All three flavours of the complementary build: at most 128 VGPRs, no scratch, the dynamic LDS size is the launcher's
    (shared with the general build), so two 512-thread workgroups per CU remain."""
    import kernel_resources
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    ks = kernel_resources.kernels(_hip.LIB_PATH)
    for flags in ('<true, true>', '<true, false>', '<false, false>'):
        names = [n for n in ks if 'welch4096ws_compl_kernel' + flags + '(' in n.replace('oth::', '')]
        assert len(names) == 1, (flags, names)
        k = ks[names[0]]
        assert k['vgpr'] + k['agpr'] <= 128 and k['scratch'] == 0 and k['spill_vgpr'] == 0, (flags, k)
