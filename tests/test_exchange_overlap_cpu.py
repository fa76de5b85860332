"""Where the exchange-2 stores of welch4096ws's complementary-window kernels sit among the consumer's arithmetic, read from
the code objects inside the built library (no GPU), with the helpers and the loop definitions of
test_hot_loop_budget_cpu.py.

The consumer ends pass 2 with sixteen rotated butterfly outputs going to LDS (exchange 2), in front of pass 3's reads.
Its four waves run in lockstep from the step's barrier; with all sixteen stores behind the last rotation their bursts
reach the CU's store path together, in front of the first counted wait of pass 3.  dft16_layer2_scatter_sym
(fft4096.hip.h) issues the stores of one radix-4 group while the next group's butterfly runs, so only the last group's
four are left behind the arithmetic.  Checked here, for flavours (1, 1) and (1, 0), on the consumer's main loop per
segment, a ds_write2_b64 counting as two stores:
  * exactly sixteen 8-byte exchange stores to sixteen different places - nothing is stored twice - and no other
    8-byte LDS store;
  * at most four of them behind the last VALU instruction in front of the first exchange-2 ds_read_b64;
  * no run of more than four without a VALU instruction between them.
The exchange stores of a segment are its 8-byte LDS stores through the address register most of them use.

The PRODUCER's exchange 1 (fifteen ds_write_b64 back to back in front of the barrier) is held to nothing here: the same
pipeline was built for it and measured slower at every placement of the wave priority
(profiles/ab_headline_exchange_overlap.txt), so its code is the parent's.

This test FAILS on the parent of the change that added it: there the consumer issues seven ds_write2_b64 (fourteen
stores) back to back in front of its exchange-2 reads.
"""
import collections
import re

import pytest

from test_hot_loop_budget_cpu import VMEM, _find, _kernels, _loops

LAST_GROUP = 4      # outputs of the last radix-4 butterfly of a 16-point transform


def _stores(ins, order):
    """-> {address register: [(position in order, [byte offsets])]} of the 8-byte LDS stores"""
    out = collections.defaultdict(list)
    for pos, k in enumerate(order):
        op, args, _ = ins[k]
        if op == 'ds_write_b64':
            m = re.search(r'offset:(\d+)', args)
            out[args.split(',')[0].strip()].append((pos, [int(m.group(1)) if m else 0]))
        elif op in ('ds_write2_b64', 'ds_write2st64_b64'):
            unit = 8 * (64 if 'st64' in op else 1)
            m0, m1 = re.search(r'offset0:(\d+)', args), re.search(r'offset1:(\d+)', args)
            out[args.split(',')[0].strip()].append((pos, [unit * int(m0.group(1)) if m0 else 0, unit * int(m1.group(1)) if m1 else 0]))
    return out


def check_segment(ins, order, wait_at, other_stores):
    """order: a segment's instruction indices as executed; wait_at(order, last store position) -> position of the wait"""
    groups = _stores(ins, order)
    assert groups, 'no 8-byte LDS store'
    reg = max(groups, key=lambda r: sum(len(o) for _, o in groups[r]))
    exch = groups[reg]
    rest = sum(len(o) for r in groups if r != reg for _, o in groups[r])
    assert rest <= other_stores, (reg, dict(groups))
    offsets = [o for _, offs in exch for o in offs]
    assert len(offsets) == 16 and len(set(offsets)) == 16, (reg, sorted(offsets))
    is_valu = [ins[k][0].startswith('v_') for k in order]
    wait = wait_at(order, exch[-1][0])
    assert wait > exch[-1][0], (wait, exch[-1])
    last_valu = max(p for p in range(wait) if is_valu[p])
    behind = sum(len(offs) for p, offs in exch if p > last_valu)
    runs, run, prev = [], 0, None
    for p, offs in exch:
        if prev is not None and any(is_valu[prev + 1:p]):
            runs.append(run)
            run = 0
        run += len(offs)
        prev = p
    runs.append(run)
    print('exchange stores through %s: %d behind the last VALU instruction, runs %s' % (reg, behind, runs))
    assert behind <= LAST_GROUP, (behind, runs)
    assert max(runs) <= LAST_GROUP, runs


def consumer_segment(ins, labels):
    """the main loop of test_hot_loop_budget_cpu.hot_loops() without the idle-step loops, from its barrier round the back edge"""
    cons = [l for l in _loops(ins, labels) if not any(ins[k][0].startswith(VMEM) for k in range(l[0], l[1] + 1))]
    assert cons
    main = max(cons, key=lambda l: l[1] - l[0])
    idle = set()
    for l in cons:
        if l != main:
            idle.update(range(l[0], l[1] + 1))
    path = [k for k in range(main[0], main[1] + 1) if k not in idle]
    bars = [k for k in path if ins[k][0] == 's_barrier']
    assert len(bars) == 1, bars
    return [k for k in path if k > bars[0]] + [k for k in path if k <= bars[0]]


def _first_read(ins):
    def at(order, last_store):
        reads = [p for p in range(last_store, len(order)) if ins[order[p]][0] == 'ds_read_b64']
        assert reads, 'no exchange-2 read behind the stores'
        return reads[0]
    return at


@pytest.mark.parametrize('flags', [(1, 1), (1, 0)])
def test_exchange_2_stores_are_spread_over_the_last_butterfly_layer(flags):
    ins, labels = _find(_kernels(), 'welch4096ws_compl_kernel', flags)
    check_segment(ins, consumer_segment(ins, labels), _first_read(ins), other_stores=0)
