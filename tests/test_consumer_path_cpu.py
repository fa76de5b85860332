"""What a data segment really executes on welch4096ws's consumer side, read from the code objects inside the built library
(no GPU).  test_hot_loop_budget_cpu.py subtracts every instruction that lies between the idle loop's head and its back
edge; a loop-header block that the data path runs through on every step (phi copies, the compares on the item word) falls
inside that span and is not counted there.  Here the path is followed through the control-flow graph instead.

The main loop is the budget test's: the largest backward branch on the consumer side (no vector-memory instruction) that
spans an s_barrier; the smaller ones are idle-step loops.  The executed path of a data segment is every instruction that
lies on some way from the main loop's head to its back edge which does not take an idle loop's s_barrier - a data step
takes exactly one barrier, the main one.  Blocks that are reached only through an idle barrier (the idle loop's own
step, its exit edge) are left out, header blocks are not.  That leaves the second instance of pass 2, on the idle loop's
exit edge, UNCHECKED here: it runs once per idle step (a one-segment chunk under the dynamic schedule), holds the copies
the data path is rid of, and is held to no count, copy or wait check; tests/test_consumer_path_gpu.py runs it.

On that path, for the detrending flavours (1, 1) and (1, 0) of both welch4096ws kernels:
  * at most PATH_VALU vector-ALU instructions.  This counter reads 426 on the parent of the change that added this file -
    the 407 the budget test counts, sixteen register copies, two compares on the item word and one more instruction in
    the loop header - and 406 with it: the copies are gone, the item word is compared in scalar registers after one
    v_readfirstlane, and the two read batches no longer start with a v_mov of a dummy operand;
  * no v_mov_b32 vN, vM at all;
  * two batches of sixteen ds_read_b64 (exchange 1 behind the barrier, exchange 2), and between the barrier resp. the
    batch's first read and the lgkmcnt(0) that closes the batch no s_waitcnt but the four hand-counted ones
    (lgkmcnt 12, 8, 4, 0): a compiler-inserted wait for a read issued in front of the batch voids the counted ones.
The same wait pattern is asked of the consumer's first step in front of the loop.

csd4096ws (both flavours) is held to the same wait pattern, to the 527 instructions it reaches (559 on the parent, with 36
copies) and to the four copies it keeps: scatter_pow16's opaque copies of the two loop-invariant twiddles W, W^4, which
keep their thirteen products from being hoisted into registers the 32 accumulators leave no room for.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

VMEM = ('global_', 'buffer_', 'flat_', 'scratch_')
PATH_VALU = 406          # reached; 409 = 407 (the body, test_hot_loop_budget_cpu.py) + two compares was the aim
CSD_PATH_VALU, CSD_COPIES = 527, 4
COUNTED = [12, 8, 4, 0]


def _kernels():
    import isa_async_hazard
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    out = {}
    for name, ins, labels in isa_async_hazard.objdump_kernels(_hip.LIB_PATH, skip_objects_with=(b'any_fft_kernel',)):
        if 'welch4096ws' in name or 'csd4096ws' in name:
            out[name] = (ins, labels)
    return out


def _is_branch(op):
    return op.startswith('s_cbranch') or op == 's_branch'


def _loops(ins, labels):
    """-> [(head, back edge)] of every backward branch that spans an s_barrier"""
    out = []
    for i, (op, args, _) in enumerate(ins):
        if _is_branch(op):
            t = labels.get(args.strip())
            if t is not None and t <= i and any(ins[k][0] == 's_barrier' for k in range(t, i + 1)):
                out.append((t, i))
    return out


def _succ(ins, labels, k):
    op, args, _ = ins[k]
    if op == 's_endpgm':
        return []
    if _is_branch(op):
        t = labels.get(args.strip())
        out = [t] if t is not None else []
        if op != 's_branch' and k + 1 < len(ins):
            out.append(k + 1)
        return out
    return [k + 1] if k + 1 < len(ins) else []


def consumer_path(ins, labels):
    """-> (sorted instruction indices of a data segment's path, main loop (head, back edge), idle barriers)"""
    cons = [l for l in _loops(ins, labels) if not any(ins[k][0].startswith(VMEM) for k in range(l[0], l[1] + 1))]
    assert cons
    main = max(cons, key=lambda l: l[1] - l[0])
    blocked = set()
    for a, b in cons:
        if (a, b) != main and b - a < main[1] - main[0]:
            blocked.update(k for k in range(a, b + 1) if ins[k][0] == 's_barrier')
    # a loop nested in the main one shares its barrier with it only if it IS the data path; the main loop needs one left
    main_barriers = [k for k in range(main[0], main[1] + 1) if ins[k][0] == 's_barrier' and k not in blocked]
    assert len(main_barriers) == 1, (main, main_barriers, sorted(blocked))
    head, back = main
    succ = {}
    fwd, todo = set(), [head]
    while todo:
        k = todo.pop()
        if k in fwd or k in blocked:
            continue
        fwd.add(k)
        nxt = [s for s in _succ(ins, labels, k) if not (k == back and s == head)]
        succ[k] = nxt
        todo.extend(nxt)
    pred = {}
    for k, nxt in succ.items():
        for s in nxt:
            pred.setdefault(s, []).append(k)
    bwd, todo = set(), [back]
    while todo:
        k = todo.pop()
        if k in bwd or k not in fwd:
            continue
        bwd.add(k)
        todo.extend(pred.get(k, []))
    return sorted(bwd), main, sorted(blocked)


def _lgkm(args):
    m = re.search(r'lgkmcnt\((\d+)\)', args)
    return int(m.group(1)) if m else None


def batch_waits(ins, seq, start, from_start):
    """seq: instruction indices in program order, start: position in seq to scan from.  Finds the next sixteen ds_read_b64
    and -> (every s_waitcnt operand string from seq[start] (from_start: seq[start] is right behind the barrier) or from
    the batch's first read to the first lgkmcnt(0) behind the sixteenth read, position behind that wait); None when
    there is no further batch."""
    waits, reads = [], 0
    for pos in range(start, len(seq)):
        op, args, _ = ins[seq[pos]]
        if op.startswith('ds_read_b64'):
            if reads == 0 and not from_start:
                waits = []
            reads += 1
        elif op == 's_waitcnt':
            waits.append(args.strip())
            if reads >= 16 and _lgkm(args) == 0:
                return waits, pos + 1
    return None


def _counted_only(waits):
    return [_lgkm(w) for w in waits] == COUNTED and all(re.fullmatch(r'lgkmcnt\(\d+\)', w) for w in waits)


def analyse(ins, labels):
    path, main, idle_barriers = consumer_path(ins, labels)
    valu = [k for k in path if ins[k][0].startswith('v_')]
    copies = [k for k in valu if ins[k][0].startswith('v_mov_b32') and re.fullmatch(r'v\d+, v\d+', ins[k][1].strip())]
    # the path in execution order: from the barrier round the back edge to the barrier again
    bar = [k for k in path if ins[k][0] == 's_barrier']
    assert len(bar) == 1, bar
    order = [k for k in path if k > bar[0]] + [k for k in path if k < bar[0]]
    batches, pos = [], 0
    while True:
        got = batch_waits(ins, order, pos, pos == 0)
        if got is None:
            break
        batches.append(got[0])
        pos = got[1]
    # the consumer's first step, in front of the loop: the last barrier above the main loop's head that no
    # vector-memory instruction separates from it, scanned in program order
    first = None
    for k in range(main[0] - 1, -1, -1):
        if ins[k][0].startswith(VMEM):
            break
        if ins[k][0] == 's_barrier':
            first = batch_waits(ins, list(range(k + 1, main[0] + 1)), 0, True)
            break
    return dict(valu=len(valu), copies=[(ins[k][0], ins[k][1]) for k in copies], batches=batches,
                first=first[0] if first else None, main=main, idle_barriers=idle_barriers)


def _find(ks, kernel, flags):
    names = [n for n in ks if re.search(r'\d+%sI%sE' % (kernel, ''.join('Lb%dE' % f for f in flags)), n)]
    assert len(names) == 1, (kernel, flags, sorted(ks))
    return ks[names[0]]


@pytest.fixture(scope='module')
def kernels():
    return _kernels()


@pytest.mark.parametrize('kernel', ['welch4096ws_compl_kernel', 'welch4096ws_kernel'])
@pytest.mark.parametrize('flags', [(1, 1), (1, 0)])
def test_consumer_data_path_has_no_copies_and_no_stray_wait(kernels, kernel, flags):
    """The executed path of a data segment (module docstring): at most 406 VALU instructions - this counter reads 426 on
    the parent, 407 + 16 copies + 2 compares + 1 -, none of them a register-to-register v_mov_b32, and only the four
    hand-counted waits inside the exchange-1 and the exchange-2 read batch, in the loop and in the consumer's first step."""
    r = analyse(*_find(kernels, kernel, flags))
    print('%s%s: %s' % (kernel, flags, r))
    assert r['valu'] <= PATH_VALU, r
    assert r['copies'] == [], r
    assert len(r['batches']) == 2, r
    for waits in r['batches']:
        assert _counted_only(waits), r
    assert r['first'] is not None and _counted_only(r['first']), r


@pytest.mark.parametrize('flags', [(1, 1), (1, 0)])
def test_two_channel_consumer_data_path(kernels, flags):
    """csd4096ws: the same wait pattern in both read batches and in the first step; 527 VALU instructions on the executed
    path (559 on the parent) and the four copies scatter_pow16 asks for (36 on the parent)."""
    r = analyse(*_find(kernels, 'csd4096ws_kernel', flags))
    print('csd4096ws_kernel%s: %s' % (flags, r))
    assert r['valu'] <= CSD_PATH_VALU and len(r['copies']) <= CSD_COPIES, r
    assert len(r['batches']) == 2, r
    for waits in r['batches']:
        assert _counted_only(waits), r
    assert r['first'] is not None and _counted_only(r['first']), r
