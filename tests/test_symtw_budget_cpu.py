"""Instruction budget of welch4096ws's complementary-window kernels with the three-shear twiddles on signed digits, read
from the code objects inside the built library (no GPU), by the method and with the helpers of
test_hot_loop_budget_cpu.py.

Per twiddle layer fifteen rotations cost three v_fma_f32 each instead of cmul's four instructions (-15), the producer no
longer forms W^14 and W^15 (-8) and the consumer corrects one bin instead of two (-6): 44 fewer than the parent's 277
(producer, per barrier) + 406 (consumer, per segment) by the source.  The built values are pinned; their sum has to lie
at least 36 below the parent's - eight are allowed for table addressing the compiler may add.
"""
import os

import pytest

from test_hot_loop_budget_cpu import _find, _kernels, hot_loops

PARENT = 277 + 406
# flavour (DETREND, PILOT) -> (producer VALU per trip of its hot loop - two segments, two barriers -, consumer VALU per
# segment) as built
BUILT = {(1, 1): (504, 385), (1, 0): (505, 385)}


@pytest.mark.parametrize('flags', sorted(BUILT))
def test_complementary_kernels_hold_the_three_shear_budget(flags):
    prod, cons = hot_loops(*_find(_kernels(), 'welch4096ws_compl_kernel', flags))
    print('welch4096ws_compl_kernel%s: producer %s, consumer %s' % (flags, prod, cons))
    want_prod, want_cons = BUILT[flags]
    assert prod['barriers'] == 2 and prod['valu'] == want_prod, prod
    assert cons['valu'] == want_cons, cons
    assert prod['scratch'] == 0 and cons['scratch'] == 0 and cons['vmcnt'] == 0
    assert want_prod / 2.0 + want_cons <= PARENT - 36


def test_complementary_kernels_fit_two_workgroups_per_cu():
    import kernel_resources
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    ks = kernel_resources.kernels(_hip.LIB_PATH)
    for flags in ('<true, true>', '<true, false>'):
        names = [n for n in ks if 'welch4096ws_compl_kernel' + flags + '(' in n.replace('oth::', '')]
        assert len(names) == 1, (flags, names)
        k = ks[names[0]]
        assert k['vgpr'] + k['agpr'] <= 128 and k['scratch'] == 0 and k['spill_vgpr'] == 0, (flags, k)
