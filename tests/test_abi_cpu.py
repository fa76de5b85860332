"""CPU-side checks of the drop-in boundary: the shared library loads, exports every
symbol include/ofdm_tools_hip.h declares, and refuses to compute without a GPU
(no silent fallback).  No compute calls are made here."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ofdm_tools_hip.h')


def product_lib(path):
    """The built library through plain ctypes, torch imported first - _hip.load()'s rule of one HIP runtime per process:
    a library loaded before torch pulls the system runtime in next to torch's, and on a GPU machine the GPU tests later
    in the same pytest process then find no device."""
    import torch  # noqa: F401
    return ctypes.CDLL(path)


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(oth_[a-z0-9_]+)\s*\(', src)))


def test_header_declares_the_expected_surface():
    names = declared_symbols()
    for must in ('oth_ctx_create', 'oth_welch_plan', 'oth_welch_exec', 'oth_welch_accumulate',
                 'oth_welch_finalize', 'oth_csd_exec', 'oth_chain_push', 'oth_channel_power', 'oth_xcorr',
                 'oth_last_error', 'oth__debug_live_resources'):
        assert must in names
    assert len(names) >= 40


def test_library_exports_every_declared_symbol():
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet (run __graft_entry__.build())')
    lib = product_lib(_hip.LIB_PATH)
    missing = [n for n in declared_symbols() if not hasattr(lib, n)]
    assert not missing, missing


def test_ctypes_table_matches_header():
    from ofdm_tools import _hip
    assert sorted(_hip.SIGNATURES) == declared_symbols()


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    assert _hip.load().oth_abi_version() == 6
    with pytest.raises(_hip.HipError) as ei:
        _hip.Context(0)
    assert ei.value.code == -2 and 'no CPU fallback' in str(ei.value)
    from ofdm_tools import ofdm_cr_tools as T
    import numpy as np
    with pytest.raises(_hip.HipError):
        T.welch_power_estimate(np.zeros(8192, np.complex64), 4096, 1.0)


def test_live_resources_are_zero_without_a_context():
    """oth__debug_live_resources needs no context and no device; a process that never created a context holds nothing.
    Run in a process of its own: on a GPU machine other modules of this pytest process keep contexts alive."""
    import subprocess
    import sys
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    code = ('import ctypes as C; from ofdm_tools import _hip; lib = _hip.load(); n = [C.c_int(-1) for _ in range(3)]; '
            'assert lib.oth__debug_live_resources(*[C.byref(v) for v in n]) == 0; '
            'assert lib.oth__debug_live_resources(None, None, None) == 0; '
            'assert _hip.live_resources() == (0, 0, 0); print([v.value for v in n])')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'gr-ofdm_tools_amd')] + sys.path),
               OFDM_TOOLS_HIP_STANDALONE='1')      # (no torch import: nothing here touches a device)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == '[0, 0, 0]', out.stdout + out.stderr


def test_exception_barrier_of_the_abi_host_files(tmp_path):
    """include/ofdm_tools_hip.h: "nothing throws or aborts".  A C++ exception below an entry point must come back as
    an error code (a bad_alloc crossing ctypes would be std::terminate and take the flowgraph down).  The barrier is the
    OTH_TRY / OTH_CATCH pair of csrc/abi_barrier.h; csrc/barrier_probe.cpp puts the SAME macros around an entry point
    that raises on request and is built here with g++ (no GPU, no HIP) - the product library carries no such hook
    (round 5's oth__debug_throw is gone from it, and so are the stamp / tail readers of the diagnostic kernel builds)."""
    import subprocess
    from ofdm_tools import _hip
    csrc = os.path.join(ROOT, 'gr-ofdm_tools_amd', 'csrc')
    so = str(tmp_path / 'barrier_probe.so')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-shared', '-fPIC', os.path.join(csrc, 'barrier_probe.cpp'), '-o', so])
    probe = ctypes.CDLL(so)
    probe.oth_probe_throw.restype = ctypes.c_int
    probe.oth_probe_last_error.restype = ctypes.c_char_p
    assert probe.oth_probe_throw(-1) == 0
    assert probe.oth_probe_throw(0) == -4 and b'memory' in probe.oth_probe_last_error()
    assert probe.oth_probe_throw(1) == -6 and probe.oth_probe_last_error() == b'debug: runtime_error'
    assert probe.oth_probe_throw(2) == -6 and b'unknown C++ exception' in probe.oth_probe_last_error()
    assert probe.oth_probe_throw(3) in (-4, -6)             # a real over-sized std::vector, not a staged throw
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    lib = product_lib(_hip.LIB_PATH)
    lib.oth_strerror.restype = ctypes.c_char_p
    assert b'internal' in lib.oth_strerror(-6)
    # the product library exports exactly what the header declares - every defined dynamic symbol, of any type and
    # name: no undeclared diagnostic hooks, no launchers, kernel stubs or handles, no host helpers
    out = subprocess.run(['nm', '-D', '--defined-only', _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert exported == sorted(_hip.SIGNATURES), set(exported) ^ set(_hip.SIGNATURES)
    # and every extern "C" body in the host files of the ABI sits inside the barrier
    bodies, defined = [], []
    for path in sorted(glob.glob(os.path.join(ROOT, 'gr-ofdm_tools_amd', 'csrc', 'abi_*.hip'))):
        src = open(path).read()
        ext = src[src.index('extern "C" {'):] if 'extern "C" {' in src else ''      # (abi_any.hip has no entry point)
        bodies += re.findall(r'^int (oth_\w+)\([^)]*\) \{\n(.*?)^\}', ext, flags=re.S | re.M)
        defined += re.findall(r'^[A-Za-z_][\w ]*[\w*] ?\*?(oth_\w+)\([^;{]*\) \{', ext, flags=re.M)
    assert len(bodies) >= 55
    for name, body in bodies:
        assert body.lstrip().startswith('OTH_TRY') and 'OTH_CATCH(' in body.rstrip().splitlines()[-1], name
    # one definition of every header symbol across those files
    assert all(defined.count(name) == 1 for name in _hip.SIGNATURES), \
        {name: defined.count(name) for name in _hip.SIGNATURES if defined.count(name) != 1}


def test_row_layouts_are_permutations(tmp_path):
    """csrc/row_layout.h is the one place that knows where a bin sits in a partial-sum row; bin_pos is what the finalize
    kernels call, here built for the host with g++ (csrc/row_layout_probe.cpp).  For every layout at the size or sizes its
    writer runs it is a bijection of [0, nfft); the digit swap of layouts 1 - 3 is its own inverse; and three positions per layout hold the bin the header's formula gives, worked out by hand.  The writers themselves are
    checked by the GPU parity tests only."""
    import subprocess
    import numpy as np
    csrc = os.path.join(ROOT, 'gr-ofdm_tools_amd', 'csrc')
    so = str(tmp_path / 'row_layout_probe.so')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-shared', '-fPIC', os.path.join(csrc, 'row_layout_probe.cpp'), '-o', so])
    probe = ctypes.CDLL(so)

    def bins(layout, nfft, l1=0, l2=0):
        return np.array([probe.oth_probe_bin_pos(pos, layout, l1, l2) for pos in range(nfft)])

    assert [probe.oth_probe_w16k_layout(n) for n in (16384, 8192)] == [2, 3]
    assert [probe.oth_probe_x1_layout(n) for n in (16384, 8192)] == [4, 5]
    assert [probe.oth_probe_w32k_layout(n) for n in (32768, 65536)] == [7, 8]
    # (layout, nfft, l1, l2): 6 at the split any_describe (fft_any.hip) gives 32768 points, L1 = 256 rows of L2 = 128
    cases = [(0, 64, 0, 0), (0, 999, 0, 0), (1, 4096, 0, 0), (2, 16384, 0, 0), (4, 16384, 0, 0), (3, 8192, 0, 0), (5, 8192, 0, 0),
             (6, 32768, 256, 128), (7, 32768, 0, 0), (8, 65536, 0, 0)]
    table = {}
    for layout, nfft, l1, l2 in cases:
        k = table[layout, nfft] = bins(layout, nfft, l1, l2)
        assert np.array_equal(np.sort(k), np.arange(nfft)), (layout, nfft)
    # the digit swap k0 <-> k1 is its own inverse: layout 1 as a whole; in layouts 2 / 3 the swap inside each block of 4096
    # positions (block k' holds the bins k' + F q, F = 4 / 2, at the layout-1 position of q - as a whole permutation they
    # are no involution: k' moves from the top of the position to the bottom of the bin)
    swap = table[1, 4096]
    assert np.array_equal(swap[swap], np.arange(4096))
    for layout, nfft, F in ((2, 16384, 4), (3, 8192, 2)):
        pos, k = np.arange(nfft), table[layout, nfft]
        assert np.array_equal(k % F, pos >> 12) and np.array_equal(swap[k // F], pos & 4095), layout
    # position -> bin, from the formulas in row_layout.h
    literal = {
        (0, 999): {0: 0, 500: 500, 998: 998},
        # 16 k0 + k1 + 256 k2 holds k0 + 16 k1 + 256 k2
        (1, 4096): {1: 16, 16 * 3 + 5 + 256 * 7: 3 + 16 * 5 + 256 * 7, 4095: 4095},
        # 4096 k' + (layout-1 position of q) holds k' + 4 q; 8192 points: k' + 2 q
        (2, 16384): {1: 4 * 16, 4096 * 3 + 16 * 2 + 9 + 256 * 5: 3 + 4 * (2 + 16 * 9 + 256 * 5), 16383: 16383},
        (3, 8192): {1: 2 * 16, 4096 + 16 * 2 + 9 + 256 * 5: 1 + 2 * (2 + 16 * 9 + 256 * 5), 8191: 8191},
        # 1024 k2 + 64 k0 + 4 k1 + q holds k0 + 16 k1 + 256 k2 + 4096 bitrev2(q)
        (4, 16384): {1: 8192, 2: 4096, 1024 * 6 + 64 * 11 + 4 * 13 + 3: 11 + 16 * 13 + 256 * 6 + 4096 * 3},
        # 512 k2 + 64 (k0 >> 1) + 4 (8 (k0 & 1) + k1) + q holds k0 + 16 k1 + 128 k2 + 2048 bitrev2(q)
        (5, 8192): {1: 4096, 32: 1, 512 * 9 + 64 * 6 + 4 * (8 + 5) + 2: 13 + 16 * 5 + 128 * 9 + 2048 * 1},
        # k1 l2 + k2 holds k1 + l1 k2
        (6, 32768): {1: 256, 128: 1, 200 * 128 + 77: 200 + 256 * 77},
        # halves of 16384 positions in layout 4: A holds bin 2 k, B bin 2 k + 1
        (7, 32768): {1: 2 * 8192, 16384: 1, 16384 + 1024 * 6 + 64 * 11 + 4 * 13 + 3: 2 * (11 + 16 * 13 + 256 * 6 + 4096 * 3) + 1},
        # halves of 32768 positions in layout 7: the first the even bins, the second the odd
        (8, 65536): {1: 4 * 8192, 32768: 1, 32768 + 16384 + 2: 2 * (2 * 4096 + 1) + 1},
        (0, 64): {0: 0, 31: 31, 63: 63},
    }
    assert sorted(literal) == sorted(table)
    for key, want in literal.items():
        assert len(want) == 3 and {pos: int(table[key][pos]) for pos in want} == want, key


def test_bench_gpus_n_without_a_gpu_exits_with_the_clear_message():
    """`python bench.py --gpus N` is the driver's command shape: without a launcher it must decide BEFORE touching the
    GPU whether it can spawn its ranks, and say why not."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip('GPU present')
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    for extra in ([], ['--gpus', '2']):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '1'] + extra, env=env,
                           capture_output=True, timeout=300)
        assert p.returncode != 0 and b'needs an MI355X' in p.stderr and b'no CPU fallback' in p.stderr, p.stderr
        assert p.stdout.strip() == b''


def test_missing_library_fails_loudly(monkeypatch):
    from ofdm_tools import _hip
    monkeypatch.setattr(_hip, '_lib', None)
    monkeypatch.setattr(_hip, 'LIB_PATH', '/nonexistent/libofdmtools_hip.so')
    with pytest.raises(_hip.HipUnavailable):
        _hip.load()


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'gr-ofdm_tools_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                text = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in text.replace('oracle/', ''), f
                assert 'import scipy' not in text and 'from scipy' not in text, f


def test_launch_recipes_table():
    """Routing as data (round 4 verdict, weak 7): which kernel build, detrend form, pilot, schedule, chunk sizes, grid
    and partial-row layout a launch takes is resolve_recipe() in csrc/abi_route.hip - pure host logic, enumerated here
    without a GPU through oth__debug_recipe (resident workgroups per CU from the built-in MI355X table; the GPU suite compares
    that table with the occupancy calculator).  Pinned twice: a readable table of 1806 recipes
    (tests/golden/recipes_small.txt) and the digest of the full enumeration of 20074 (nfft x nperseg x overlap x window
    class x detrend mode x one / two channels x segment count x streams).  An intended routing change regenerates both
    with `python tests/recipes.py --write`; the diff of the small table is the review."""
    import recipes
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    lib = recipes._lib()
    small = recipes.table(lib, False)
    want = open(os.path.join(ROOT, 'tests', 'golden', 'recipes_small.txt')).read().splitlines()
    assert len(small) == len(want)
    diff = [(a, b) for a, b in zip(small, want) if a != b]
    assert not diff, diff[:3]
    full = recipes.table(lib, True)
    pinned = open(os.path.join(ROOT, 'tests', 'golden', 'recipes_full.sha256')).read().split()
    assert (recipes.digest(full), len(full)) == (pinned[0], int(pinned[1]))

    def fields(**kw):
        return dict(f.split('=') for f in recipes.recipe(lib, **kw).split())
    # the BASELINE configurations
    c2 = fields(nfft=4096, nperseg=4096, noverlap=2048, nseg=131071)
    assert (c2['kernel'], c2['form'], c2['pilot'], c2['sched'], c2['chunk'], c2['W']) == ('welch4096:ws', 'freq', 'inline', 'dynamic', '20', '512')
    c3 = fields(nfft=4096, nperseg=4096, noverlap=2048, two_channel=1, nseg=32767)
    assert (c3['kernel'], c3['pilot'], c3['sched'], c3['W'], c3['nch']) == ('csd4096ws', 'inline', 'contiguous', '256', '4')
    c4 = fields(nfft=4096, nperseg=1024, noverlap=512, nseg=65535)                # the sweeper's own call (spectrum_sweeper.py:263)
    assert (c4['kernel'], c4['form'], c4['pilot']) == ('welch4096:dpp', 'time', 'launch')
    c5 = fields(nfft=16384, nperseg=16384, noverlap=0, window=0, detrend=0, nseg=256, nstreams=64)
    assert (c5['kernel'], c5['sched'], c5['layout'], c5['W']) == ('welch16k1x:pipe', 'contiguous', '4', '4')
    # round 6: every other length (csrc/fft_any.hip, fft_tl.hip) - and what is still refused, with the reason
    for n, kind in ((8, 'direct'), (1000, 'direct'), (15000, 'direct'), (1021, 'bluestein'), (8191, 'bluestein'), (10007, 'bluestein2'),
                    (20000, 'bluestein2'), (32768, 'onewg'), (65536, 'onewg'), (131072, 'twolevel'), (1048576, 'twolevel')):
        f = fields(nfft=n, nperseg=n, noverlap=n // 2)
        assert (f['kernel'], f['form'], f['pilot'], f['layout']) == ('anyfft:' + kind, 'time', 'none', ('8' if n == 65536 else '7') if kind == 'onewg' else ('6' if 'twolevel' in kind else '0')), n
    assert fields(nfft=65536, nperseg=65536, noverlap=32768, two_channel=1)['kernel'] == 'anyfft:twolevel:r16'
    assert fields(nfft=65536, nperseg=65536, noverlap=32768, variant='anycov')['kernel'] == 'anyfft:twolevel'
    assert fields(nfft=32768, nperseg=32768, noverlap=16384, variant='r16')['kernel'] == 'anyfft:twolevel:r16'
    assert fields(nfft=65536, nperseg=65536, noverlap=32768, variant='r16')['kernel'] == 'anyfft:twolevel:r16'
    assert fields(nfft=65536, nperseg=65536, noverlap=32768, nseg=1000)['W'] == '128'      # a pair of workgroups per segment
    assert fields(nfft=32768, nperseg=32768, noverlap=16384, two_channel=1)['kernel'] == 'anyfft:twolevel:r16'
    assert fields(nfft=32768, nperseg=8192, noverlap=4096)['kernel'] == 'anyfft:twolevel:r16'      # zero-padded segments
    for n in (2097152, 524290, 600000):
        assert '1048576' in recipes.recipe(lib, nfft=n, nperseg=n, noverlap=0), n
    assert recipes.recipe(lib, nfft=1000, nperseg=1000, noverlap=500, kernel=2).startswith('error -3')
    # a launch of fewer than eight segments detrends before the window in BOTH modes; FAST has no pilot
    for det in (1, 3):
        few = fields(nfft=4096, nperseg=4096, noverlap=2048, detrend=det, nseg=7)
        assert (few['kernel'], few['form']) == ('welch4096:pipe', 'time')
        assert few['pilot'] == ('launch' if det == 1 else 'none')
    # a window without a confined spectrum, other steps, the coverage kernel, an unsupported request
    assert fields(nfft=4096, nperseg=4096, noverlap=2048, window=2)['kernel'] == 'welch4096:pipe'
    assert fields(nfft=4096, nperseg=4096, noverlap=3072)['kernel'] == 'welch4096:dpp'
    assert fields(nfft=16384, nperseg=16384, noverlap=8192)['kernel'] == 'welch16k1x_half'
    assert fields(nfft=16384, nperseg=16384, noverlap=8192, window=2)['kernel'] == 'welch16k'
    assert fields(nfft=1024, nperseg=1024, noverlap=512)['kernel'] == 'segws'
    assert fields(nfft=128, nperseg=128, noverlap=64)['kernel'] == 'welch_generic'
    assert fields(nfft=4096, nperseg=4096, noverlap=2048, kernel=1)['kernel'] == 'welch_generic'
    assert recipes.recipe(lib, nfft=128, nperseg=128, noverlap=64, kernel=2).startswith('error -3')
    # more streams than ticket words: the dynamic schedule becomes interleaved chunks
    assert fields(nfft=4096, nperseg=4096, noverlap=2048, nseg=20000, nstreams=100)['sched'] == 'interleaved'


def test_no_instruction_reads_a_register_whose_load_is_in_flight():
    """The one-exchange kernels issue sample / window / exchange loads from inline asm and wait for them with explicit
    s_waitcnt statements.  The compiler takes a register for valid from the asm that loads it: a copy it makes in front
    of the wait (a register shuffle at a loop edge, the input of an in-out operand) or an instruction it moves across a
    wait that does not name the register reads a register whose load may still be in flight - garbage, depending on
    timing.  Late in round 5 exactly that was found in the shipped 16384 / 8192 builds (the role-split 8192 kernel's
    first build failed outright; the others had only ever been lucky).  tools/isa_async_hazard.py disassembles every
    code object of the built library, follows every load to the wait that covers it along every path, and reports
    anything that touches its destination before: there must be nothing."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_async_hazard
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    found, n = [], 0
    # fft_any.hip's code object (twelve builds of any_fft_kernel, 20 000 instructions each, seven radix bodies behind a
    # switch) holds no inline asm and no hand-written wait: every load in it is the compiler's own and cannot produce a
    # finding, and disassembling it with symbolised operands alone took 260 s of this suite
    for kname, ins, labels in isa_async_hazard.objdump_kernels(_hip.LIB_PATH, skip_objects_with=(b'any_fft_kernel',)):
        if kname.startswith('_Z'):
            n += 1
            isa_async_hazard.walk(ins, labels, kname, found)
    assert n > 150, n
    assert not found, sorted(set((k[-50:], t) for k, t, _ in found))[:5]


def test_hot_kernels_have_no_scratch():
    """A spilled register comes back at memory latency in every step (12 % of the two-channel kernel in round
    2; round 4's verdict found 2-25 spilled VGPRs in five default builds).  The code objects inside the shipped library
    say what each kernel uses: the default builds of the tuned kernels must carry no scratch memory."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    ks = kernel_resources.kernels(_hip.LIB_PATH)
    hot = ['welch4096ws_kernel<true, true>', 'welch4096ws_kernel<true, false>', 'welch4096ws_kernel<false, false>',
           # welch4096.hip, both builds (any step / zero-padded segments - C4 as the reference block calls it - and the
           # 50 % pipeline for windows whose spectrum is not confined; same names, the larger figure counts)
           'welch4096_kernel<true, 16, true>', 'welch4096_kernel<true, 16, false>', 'welch4096_kernel<false, 16, false>',
           'welch4096_kernel<true, 4, true>', 'welch4096_kernel<true, 4, false>',
           'csd4096ws_kernel<true, true>', 'csd4096ws_kernel<true, false>',
           'welch16k1x_pipe_kernel<16, false>', 'welch16k1x_pipe_kernel<8, false>',
           'welch8kws_kernel<2, true>', 'welch8kws_kernel<2, false>', 'welch8kws_kernel<0, false>',
           'welch16k1x_half_kernel<16, 2, true>', 'welch16k1x_half_kernel<16, 2, false>', 'welch16k1x_half_kernel<16, 0, false>',
           'welch16k1x_half_kernel<8, 2, true>', 'welch16k1x_half_kernel<8, 2, false>', 'welch16k1x_half_kernel<8, 0, false>',
           'segws_kernel<4, 1, true>', 'segws_kernel<8, 2, true>', 'seg_kernel<1, 0, true, false, 3, 16, true>',
           'seg_kernel<2, 0, true, false, 3, 16, true>',
           # the fused chain builds 256 ... 4096 and the whole-segment-load Welch builds at 256 / 512
           'seg_kernel<1, 1, false, true, 3, 16, false>', 'seg_kernel<2, 1, false, true, 3, 16, false>',
           'seg_kernel<4, 1, false, true, 3, 16, false>', 'seg_kernel<8, 1, false, true, 3, 16, false>',
           'seg_kernel<16, 1, false, true, 3, 16, false>', 'seg_kernel<1, 1, true, false, 3, 16, true>',
           'seg_kernel<2, 1, true, false, 3, 16, true>']
    found = {h: [n for n in ks if h + '(' in n.replace('oth::', '')] for h in hot}
    missing = [h for h, n in found.items() if len(n) != 1]
    assert not missing, missing
    bad = {h: ks[n[0]]['scratch'] for h, n in found.items() if ks[n[0]]['scratch']}
    assert not bad, bad
    # Second list (round 6): builds a default plan CAN reach that do carry scratch, each with a budget in bytes per lane -
    # so that a spill that creeps into another build, or grows, is seen.
    #   (csd4096ws_kernel<false, false>, five registers in round 5, is gone: a two-channel plan without detrend runs the
    #    detrending build on an all-zero window-spectrum table, csrc/csd4096ws.hip launch_csd_tuned4096ws)
    #   csd4096_kernel<true, true>       the one-role two-channel kernel (other steps than nfft / 2, > 2^30 segments)
    #   chain16k* / chain16k1x_kernel    the 8192 / 16384-point chain epilogues (outside the steady-state step)
    #   *_generic / pgram / xcorr <16384, 1024>, any_fft_kernel<1024, *>   COVERAGE kernels at their largest tile: 1024 threads
    #                                    hold the compiler to 128 registers; they are the comparators of the tuned-vs-generic
    #                                    tests and the route of lengths no tuned kernel takes - right first, not fast
    budget = {'csd4096_kernel<true, true>': 52,
              'chain16k_kernel<2, false, true>': 20, 'chain16k_kernel<4, false, true>': 28, 'chain16k_kernel<4, true, false>': 12,
              'chain16k1x_kernel<16, false>': 28, 'chain16k1x_kernel<16, true>': 20, 'chain16k1x_kernel<8, false>': 16,
              'chain16k1x_kernel<8, true>': 12,
              'welch_generic_kernel<16384, 1024, false>': 292, 'welch_generic_kernel<16384, 1024, true>': 668,
              'welch_generic_kernel<8192, 512, true>': 140, 'pgram_kernel<16384, 1024>': 220, 'xcorr_kernel<16384, 1024>': 392,
              # (<threads, store form, twiddles in LDS, single column>: the two-channel sums and the column tiles of the
              # 1024-thread builds; the single-column one-channel builds - every direct / Bluestein Welch plan - carry none)
              'any_fft_kernel<1024, 0, true, false>': 12, 'any_fft_kernel<1024, 1, false, false>': 44,
              'any_fft_kernel<1024, 1, true, false>': 212, 'any_fft_kernel<1024, 2, false, false>': 364,
              'any_fft_kernel<1024, 2, false, true>': 244, 'any_fft_kernel<1024, 2, true, false>': 468,
              'any_fft_kernel<1024, 2, true, true>': 244, 'any_fft_kernel<1024, 3, true, false>': 16}
    over = {}
    for h, lim in budget.items():
        names = [n for n in ks if n.replace('oth::', '').startswith(h + '(') or n.replace('oth::', '') == h]
        assert len(names) == 1, (h, names)
        if ks[names[0]]['scratch'] > lim:
            over[h] = (ks[names[0]]['scratch'], lim)
    assert not over, over
    # and nothing else in the library spills except the zero-padded seg_kernel<..., 4, ...> builds ("seg4": four waves per
    # SIMD - an A/B variant, oth_plan_set_tuning) already known
    known = set(budget) | set(hot)
    rest = {n: v['scratch'] for n, v in ks.items() if v['scratch'] and not any(n.replace('oth::', '').startswith(k) for k in known)
            and 'seg_kernel<' not in n}
    assert not rest, rest
