"""ctypes binding of libofdmtools_hip.so (include/ofdm_tools_hip.h).

The only compute back end of this package.  There is no NumPy/SciPy fallback:
if the shared library is missing or no MI355X is visible every entry point
raises :class:`HipUnavailable` / :class:`HipError` with the reason.
"""
import ctypes as C
import os
import threading

import numpy as np

OK = 0
DETREND_NONE, DETREND_CONSTANT, DETREND_CONSTANT_EXACT, DETREND_CONSTANT_FAST = 0, 1, 2, 3
SCALE_RAW, SCALE_DENSITY, SCALE_OVER_N2, SCALE_SPECTRUM = 0, 1, 2, 3
EPI_MAG, EPI_MAG2, EPI_MAG2_OVER_N2 = 0, 1, 2
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TUNED = 0, 1, 2
SCHED_CONTIGUOUS, SCHED_INTERLEAVED, SCHED_DYNAMIC = 0, 1, 2
HOSTWAIT_POLL, HOSTWAIT_SYNC = 0, 1
AVERAGE_MEAN, AVERAGE_MEDIAN = 0, 1      # oth_plan_set_average: scipy.signal.welch average='mean' / 'median'
EIG_OF_S, EIG_OF_G = 0, 1      # oth_welch_matrix_eig: the spectral matrix S, the coherence matrix G
GCC_PLAIN, GCC_PHAT, GCC_SCOT = 0, 1, 2      # oth_welch_matrix_gcc: the weighting of the generalized cross-correlation
GCC_POINTS_MAX = 16384      # upsample * nfft at most
OUT_RING = 4      # oth_plan::kOutRing: launch (ticket) t of a plan delivers into output slot t % OUT_RING

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('OFDM_TOOLS_HIP_LIB',
                          os.path.join(os.path.dirname(_HERE), 'lib', 'libofdmtools_hip.so'))


class HipUnavailable(RuntimeError):
    """libofdmtools_hip.so could not be loaded (not built, or ROCm runtime missing)."""


class HipError(RuntimeError):
    def __init__(self, code, where, detail):
        RuntimeError.__init__(self, '%s failed (%d): %s' % (where, code, detail))
        self.code = code


_p = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_f = C.POINTER(C.c_float)
_u64p = C.POINTER(C.c_uint64)
_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)
_ubp = C.POINTER(C.c_ubyte)

# name -> (restype, argtypes); must list every symbol include/ofdm_tools_hip.h declares
SIGNATURES = {
    'oth_abi_version': (C.c_int, []),
    'oth_strerror': (C.c_char_p, [C.c_int]),
    'oth_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'oth_ctx_create': (C.c_int, [C.c_int, _pp]),
    'oth_ctx_create_on_stream': (C.c_int, [C.c_int, _p, _pp]),
    'oth_ctx_destroy': (C.c_int, [_p]),
    'oth_last_error': (C.c_char_p, [_p]),
    'oth_ctx_sync': (C.c_int, [_p]),
    'oth_ctx_device_name': (C.c_int, [_p, C.c_char_p, C.c_size_t]),
    'oth_ctx_set_timing': (C.c_int, [_p, C.c_int]),
    'oth_ctx_get_timing': (C.c_int, [_p, C.POINTER(C.c_double), _u64p, C.c_int]),
    'oth_dev_alloc': (C.c_int, [_p, C.c_size_t, _pp]),
    'oth_dev_free': (C.c_int, [_p, _p]),
    'oth_memcpy_h2d': (C.c_int, [_p, _p, _p, C.c_size_t]),
    'oth_memcpy_d2h': (C.c_int, [_p, _p, _p, C.c_size_t]),
    'oth_synth_iq': (C.c_int, [_p, _p, C.c_size_t, C.c_uint64, C.c_int, _f, _f, C.c_float, C.c_float]),
    'oth_stream_read_probe': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    'oth_iq_power': (C.c_int, [_p, _p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_double)]),
    'oth_welch_plan': (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _f, C.c_int, C.c_int, C.c_double, C.c_int,
                                 C.c_int, _pp]),
    'oth_plan_destroy': (C.c_int, [_p]),
    'oth_plan_set_output_db': (C.c_int, [_p, C.c_int]),
    'oth_plan_set_kernel': (C.c_int, [_p, C.c_int]),
    'oth_plan_set_schedule': (C.c_int, [_p, C.c_int]),
    'oth_plan_out_len': (C.c_int, [_p, C.POINTER(C.c_int)]),
    'oth_plan_set_hostwait': (C.c_int, [_p, C.c_int]),
    'oth_plan_set_average': (C.c_int, [_p, C.c_int]),
    'oth_welch_segments_dev': (C.c_int, [_p, _p, C.c_size_t, _p, C.c_uint64, _u64p]),
    'oth_dpss': (C.c_int, [C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'oth_mtm_plan': (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_int, _f, _f, C.c_int, C.c_int, C.c_double, C.c_int,
                               C.c_int, _pp]),
    'oth_mtm_csd_plan': (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_int, _f, _f, C.c_int, C.c_int, C.c_double, C.c_int,
                                   C.c_int, _pp]),
    'oth_mtm_ftest_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, _p, _p, _p, _u64p]),
    'oth_mtm_ftest': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f, _f, _f, _u64p]),
    'oth_welch_sk_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, _p, _p, _u64p]),
    'oth_welch_sk': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f, _f, _u64p]),
    'oth_welch_set_cycles': (C.c_int, [_p, C.c_int, C.POINTER(C.c_double)]),
    'oth_welch_cyclic_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, _p, _p, _p, _u64p]),
    'oth_welch_cyclic': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f, _f, _f, _u64p]),
    'oth_welch_set_lags': (C.c_int, [_p, C.c_int, C.POINTER(C.c_int)]),
    'oth_welch_caf_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, _p, _p, _u64p]),
    'oth_welch_caf': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f, _f, _u64p]),
    'oth_welch_set_prototype': (C.c_int, [_p, C.c_int, _f]),
    'oth_welch_pfb_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, _p, _u64p]),
    'oth_welch_pfb': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f, _u64p]),
    'oth_welch_matrix_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, _p, _p, _u64p]),
    'oth_welch_matrix': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, _f, _f, _u64p]),
    'oth_welch_matrix_eig_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, C.c_int, _p, _p, _u64p]),
    'oth_welch_matrix_eig': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, _f, _f, _u64p]),
    'oth_welch_set_steering': (C.c_int, [_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double]),
    'oth_welch_matrix_doa_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_double, _p, _p, _p, _u64p]),
    'oth_welch_matrix_doa': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _f, _f, _f, _u64p]),
    'oth_welch_matrix_gcc_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _u64p]),
    'oth_welch_matrix_gcc': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f, _f, _u64p]),
    'oth_mtm_jackknife_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, _p, _p, _u64p]),
    'oth_mtm_jackknife': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f, _f, _u64p]),
    'oth_mtm_csd_jackknife_dev': (C.c_int, [_p, _p, _p, C.c_size_t, _p, _p, _p, _p, _u64p]),
    'oth_mtm_csd_jackknife': (C.c_int, [_p, _p, _p, C.c_size_t, C.c_int, _f, _f, _f, _f, _u64p]),
    'oth_mtm_set_ratios': (C.c_int, [_p, C.POINTER(C.c_double)]),
    'oth_mtm_adaptive_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, C.c_int, _p, _p, _u64p]),
    'oth_mtm_adaptive': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, _f, _f, _u64p]),
    'oth_plan_set_tuning': (C.c_int, [_p, C.c_char_p, C.c_int, C.c_int, C.c_int]),
    'oth_welch_exec': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f, _u64p]),
    'oth_welch_exec_async': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _u64p]),
    'oth_welch_poll': (C.c_int, [_p, C.c_uint64, _f, _u64p, C.POINTER(C.c_int)]),
    'oth_welch_wait': (C.c_int, [_p, C.c_uint64, _f, _u64p]),
    'oth_welch_exec_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, _p, _u64p]),
    'oth_welch_partial_dev': (C.c_int, [_p, _p, C.c_size_t, _p, _u64p]),
    'oth_welch_scale_dev': (C.c_int, [_p, _p, C.c_uint64, _p]),
    'oth_welch_accumulate': (C.c_int, [_p, _p, C.c_size_t]),
    'oth_welch_finalize': (C.c_int, [_p, _f, _u64p]),
    'oth_welch_reset': (C.c_int, [_p]),
    'oth_csd_exec': (C.c_int, [_p, _p, _p, C.c_size_t, C.c_int, _f, _f, _f, _f, _u64p]),
    'oth_csd_exec_dev': (C.c_int, [_p, _p, _p, C.c_size_t, _p, _p, _p, _p, _u64p]),
    'oth_csd_partial_dev': (C.c_int, [_p, _p, _p, C.c_size_t, _p, _u64p]),
    'oth_csd_scale_dev': (C.c_int, [_p, _p, C.c_uint64, _p, _p, _p, _p]),
    'oth_chain_create': (C.c_int, [_p, C.c_int, _f, C.c_int, C.c_int, C.c_int, _pp]),
    'oth_chain_destroy': (C.c_int, [_p]),
    'oth_chain_set_keep_one_in_n': (C.c_int, [_p, C.c_int]),
    'oth_chain_set_iir_log': (C.c_int, [_p, C.c_float, C.c_float]),
    'oth_chain_set_peak_hold': (C.c_int, [_p, C.c_int]),
    'oth_chain_set_kernel': (C.c_int, [_p, C.c_int]),
    'oth_chain_reset': (C.c_int, [_p]),
    'oth_chain_push': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f, C.c_size_t, _u64p]),
    'oth_chain_push_dev': (C.c_int, [_p, _p, C.c_size_t, _p, C.c_size_t, _u64p]),
    'oth_chain_push_async': (C.c_int, [_p, _p, C.c_size_t, _u64p]),
    'oth_chain_poll': (C.c_int, [_p, C.c_uint64, _f, _u64p, C.POINTER(C.c_int)]),
    'oth_chain_wait': (C.c_int, [_p, C.c_uint64, _f, _u64p]),
    'oth_chain_ticket_rows': (C.c_int, [_p, C.c_uint64, _u64p]),
    'oth_chain_last_push_ops': (C.c_int, [_p, _u64p]),
    'oth_chain_get_peak': (C.c_int, [_p, _f]),
    'oth_chain_get_iir': (C.c_int, [_p, _f]),
    'oth_channelizer_create': (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _f, _pp]),
    'oth_channelizer_destroy': (C.c_int, [_p]),
    'oth_channelizer_reset': (C.c_int, [_p]),
    'oth_channelizer_frames': (C.c_int, [_p, C.c_size_t, _u64p]),
    'oth_channelizer_pending': (C.c_int, [_p, C.POINTER(C.c_size_t)]),
    'oth_channelizer_push_dev': (C.c_int, [_p, _p, C.c_size_t, _p, C.c_size_t, _u64p]),
    'oth_channelizer_push': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _p, C.c_size_t, _u64p]),
    'oth_cp_sync_dev': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_float,
                                  C.c_size_t, _p, _p, _p, _u64p]),
    'oth_cp_sync': (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_float, C.c_size_t,
                              _p, _f, _f, _u64p]),
    'oth_rows_group_mean': (C.c_int, [_p, _f, C.c_size_t, C.c_int, C.c_int, _f]),
    'oth_channel_power': (C.c_int, [_p, _f, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    _f, _f]),
    'oth_bin_threshold': (C.c_int, [_p, _f, C.c_int, C.c_int, C.c_double, C.c_float, C.POINTER(C.c_ubyte), _f]),
    'oth_scan_decide_dev': (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_double, C.c_float, C.c_int, C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(C.c_ubyte), _f, _f]),
    'oth_scan_decide_dev_out': (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_double, C.c_float, C.c_int, C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), _p, _p, _p]),
    'oth_xcorr': (C.c_int, [_p, _p, C.c_size_t, _p, C.c_size_t, C.c_int, _f]),
    'oth_fac': (C.c_int, [_p, _p, C.c_size_t, C.c_int, _f]),
    'oth__debug_recipe': (C.c_int, [C.c_int] * 7 + [C.c_char_p, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                                    C.c_size_t]),
    'oth__debug_recipe_tuned': (C.c_int, [C.c_int] * 7 + [C.c_char_p, C.c_int, C.c_longlong] + [C.c_int] * 6 + [C.c_char_p, C.c_size_t]),
    'oth__debug_last_recipe': (C.c_int, [_p, C.c_char_p, C.c_size_t]),
    'oth__debug_channelizer_recipe': (C.c_int, [_p, C.c_char_p, C.c_size_t]),
    'oth__debug_live_resources': (C.c_int, [C.POINTER(C.c_int)] * 3),
}

_lib = None
_lib_lock = threading.Lock()


def load():
    """Load the shared library once and attach the prototypes."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 and finds no GPU if another copy
        # (the system ROCm's, which this library would pull in) was loaded first.  Multi-GPU hosts use torch for
        # device tensors and torch.distributed, so when torch is installed its runtime goes in first and this
        # library binds to it (same SONAME).  OFDM_TOOLS_HIP_STANDALONE=1 skips the import.
        if os.environ.get('OFDM_TOOLS_HIP_STANDALONE') != '1':
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        if not os.path.exists(LIB_PATH):
            raise HipUnavailable('%s not found - build it with `make -C gr-ofdm_tools_amd` '
                                 '(or __graft_entry__.build()); this package has no CPU fallback' % LIB_PATH)
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:
            raise HipUnavailable('cannot load %s: %s' % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def live_resources():
    """(device buffers, pinned host buffers, events) the library's contexts, plans and chains hold in this process right
    now (oth__debug_live_resources; needs no device)."""
    n = [C.c_int() for _ in range(3)]
    rc = load().oth__debug_live_resources(*[C.byref(v) for v in n])
    if rc != OK:
        raise HipError(rc, 'oth__debug_live_resources', load().oth_last_error(None).decode())
    return tuple(v.value for v in n)


def _c64(x):
    x = np.ascontiguousarray(x, dtype=np.complex64)
    if x.ndim != 1:
        x = x.reshape(-1)
    return x


def _fptr(a):
    return a.ctypes.data_as(_f)


def _src(x, nsamples):
    """The input of a statistic's host form -> (pointer, samples, src_is_device): a host complex64 array, or a device
    pointer when nsamples is given.  (The pointer holds on to the array it was taken from.)"""
    if nsamples is None:
        x = _c64(x)
        return x.ctypes.data_as(_p), len(x), 0
    return x, int(nsamples), 1


def _src2(x, y, nsamples):
    """_src for a pair of captures -> (pointer, pointer, samples, src_is_device)"""
    (sx, count, dev), (sy, county, _) = _src(x, nsamples), _src(y, nsamples)
    if count != county:
        raise ValueError('x and y must have the same length')
    return sx, sy, count, dev


def _channels(x, nsamples):
    """The input of the matrix family -> (pointer, samples per channel, channels, src_is_device): a host complex64 array
    (C, n), or a device pointer to [C][nsamples] when nsamples is given as (C, nsamples).  (The pointer holds on to the
    array it was taken from.)"""
    if nsamples is None:
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError('x must be a (C, n) array of C channels')
        x = np.ascontiguousarray(x, np.complex64)
        nchan, count, src, dev = x.shape[0], x.shape[1], x.ctypes.data_as(_p), 0
    else:
        nchan, count = (int(v) for v in nsamples)
        src, dev = x, 1
    if not 2 <= nchan <= 8:
        raise ValueError('the spectral matrix takes 2 ... 8 channels, not %d' % nchan)
    return src, count, nchan, dev


def _eig_of(of):
    """'S' / 'G' -> EIG_OF_S / EIG_OF_G; an integer passes as it is (the library refuses what it does not know)"""
    return {'S': EIG_OF_S, 'G': EIG_OF_G}[of] if isinstance(of, str) else int(of)


def _gcc_weighting(weighting):
    """'plain' / 'phat' / 'scot' -> GCC_PLAIN / GCC_PHAT / GCC_SCOT; an integer passes as it is (the library refuses what it
    does not know)"""
    return {'plain': GCC_PLAIN, 'phat': GCC_PHAT, 'scot': GCC_SCOT}[weighting] if isinstance(weighting, str) else int(weighting)


def gcc_pairs(nchan):
    """the pair of each row of matrix_gcc, in the rows' order: (0,1), (0,2), ..., (C-2,C-1)"""
    return [(a, b) for a in range(nchan) for b in range(a + 1, nchan)]


def unpack_matrix(packed, nchan):
    """The packed upper triangle of oth_welch_matrix, complex [C (C + 1) / 2, m] row by row -> the Hermitian [C, C, m]"""
    S = np.empty((nchan, nchan, packed.shape[-1]), packed.dtype)
    k = 0
    for a in range(nchan):
        for b in range(a, nchan):
            S[a, b] = packed[k]
            if b != a:
                S[b, a] = np.conj(packed[k])
            k += 1
    return S


class _Handle(object):
    """What Context, WelchPlan, Chain and Channelizer share: a handle self.h of the library under a context self.ctx (a
    Context has none: it is its own), and the one way their methods call it.  The prototypes of load() convert the arguments: a device pointer goes in as the
    integer it is, 0 or None for a row the caller leaves out is NULL."""

    def _call(self, name, *args):
        """lib.<name>(self.h, *args); anything but OTH_OK raises HipError under the same name"""
        ctx = getattr(self, 'ctx', self)
        ctx.check(getattr(ctx.lib, name)(self.h, *args), name)

    def _count(self, name, *args):
        """The same with a uint64_t * behind the arguments -> what the library wrote there: segments, rows, frames.  (Spelled
        out, not on top of _call: a second Python frame per call showed in the host cost, profiles/binding_fold_ab.txt.)"""
        n, ctx = C.c_uint64(), getattr(self, 'ctx', self)
        ctx.check(getattr(ctx.lib, name)(self.h, *args, C.byref(n)), name)
        return n.value


class Context(_Handle):
    """One device + one HIP stream (oth_ctx).  The library serialises calls per context, so blocks
    running on different scheduler threads may share one."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = C.c_void_p()
        if stream is None:
            rc = self.lib.oth_ctx_create(int(device), C.byref(h))
        else:
            rc = self.lib.oth_ctx_create_on_stream(int(device), int(stream), C.byref(h))
        if rc != OK:
            raise HipError(rc, 'oth_ctx_create', self.lib.oth_last_error(None).decode())
        self.h = h
        self.device = int(device)
        self.stream = None if stream is None else int(stream)      # the adopted hipStream_t, if any
        self._plans_lock = threading.Lock()

    def on_torch_stream(self):
        """True when this context runs on torch's current stream of its device: kernels and torch ops
        (collectives included) are then ordered by the stream and need no host synchronisation between them."""
        if self.stream is None:
            return False
        import torch
        return int(torch.cuda.current_stream(self.device).cuda_stream) == self.stream

    def check(self, rc, where):
        if rc != OK:
            raise HipError(rc, where, self.lib.oth_last_error(self.h).decode())

    def close(self):
        if getattr(self, 'h', None):
            for plan in self.__dict__.pop('_plans', {}).values():
                plan.close()
            self.lib.oth_ctx_destroy(self.h)
            self.h = None

    def cached_plan(self, key, make, limit=64):
        """One plan per (context, key) for callers that ask for the same shape with every request (the legacy helpers of
        ofdm_cr_tools): a plan owns device tables and scratch, and building one costs allocations and a stream
        synchronisation.  GNU Radio block threads share the default context, so the cache is locked; a hit moves to the
        young end (least-recently-used eviction), and past `limit` shapes the oldest plan WITHOUT an uncollected
        exec_async() ticket goes - a plan that still owes a result is kept even if that overshoots the limit (closing it
        would turn the ticket's poll / wait into an error inside work()).  The cache is closed with the context."""
        with self._plans_lock:
            plans = self.__dict__.setdefault('_plans', {})
            plan = plans.pop(key, None)
            if plan is None or not plan.h:
                plan = make()
            plans[key] = plan                  # (re-)inserted at the young end
            while len(plans) > limit:
                victim = next((k for k, v in plans.items() if k != key and not getattr(v, 'outstanding', 0)), None)
                if victim is None:
                    break
                plans.pop(victim).close()
            return plan

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing -------------------------------------------------------------
    def sync(self):
        self._call('oth_ctx_sync')

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._call('oth_ctx_device_name', buf, 256)
        return buf.value.decode()

    def set_timing(self, on):
        self._call('oth_ctx_set_timing', 1 if on else 0)

    def get_timing(self, reset=True):
        ms, n = C.c_double(), C.c_uint64()
        self._call('oth_ctx_get_timing', C.byref(ms), C.byref(n), 1 if reset else 0)
        return ms.value, n.value

    def alloc(self, nbytes):
        p = C.c_void_p()
        self._call('oth_dev_alloc', nbytes, C.byref(p))
        return p.value

    def free(self, ptr):
        self._call('oth_dev_free', ptr)

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._call('oth_memcpy_h2d', dptr, arr.ctypes.data_as(_p), arr.nbytes)

    def d2h(self, dptr, shape, dtype):
        out = np.empty(shape, dtype)
        self._call('oth_memcpy_d2h', out.ctypes.data_as(_p), dptr, out.nbytes)
        return out

    def synth_iq(self, dptr, nsamples, seed, tones=(), dc=0j):
        amp = np.array([t[0] for t in tones], np.float32)
        frq = np.array([t[1] for t in tones], np.float32)
        self._call('oth_synth_iq', dptr, nsamples, seed, len(tones), _fptr(amp) if len(tones) else None,
                   _fptr(frq) if len(tones) else None, float(np.real(dc)), float(np.imag(dc)))

    def stream_read_probe(self, dptr, nbytes, repeats=5):
        ms = C.c_double()
        self._call('oth_stream_read_probe', dptr, nbytes, repeats, C.byref(ms))
        return ms.value

    def iq_power(self, dptr, nsamples):
        mr, mi, var = C.c_double(), C.c_double(), C.c_double()
        self._call('oth_iq_power', dptr, nsamples, C.byref(mr), C.byref(mi), C.byref(var))
        return complex(mr.value, mi.value), var.value

    # -- factories ------------------------------------------------------------
    def welch_plan(self, nfft, nperseg=None, noverlap=None, window=None, detrend=DETREND_CONSTANT,
                   scaling=SCALE_DENSITY, fs=1.0, fftshift=False, trim_bins=0, db=False, kernel=KERNEL_AUTO,
                   average='mean'):
        """average: 'mean' (default), 'median' (scipy.signal.welch average='median') or AVERAGE_MEAN / AVERAGE_MEDIAN."""
        plan = WelchPlan(self, nfft, nperseg, noverlap, window, detrend, scaling, fs, fftshift, trim_bins, db, kernel)
        if average_code(average) != AVERAGE_MEAN:
            plan.set_average(average)
        return plan

    def mtm_plan(self, nfft, nperseg=None, noverlap=0, nw=4.0, ntapers=None, tapers=None, weights='unity',
                 detrend=DETREND_CONSTANT, scaling=SCALE_DENSITY, fs=1.0, fftshift=False, trim_bins=0, db=False):
        """Multitaper (Thomson) PSD plan (oth_mtm_plan): per segment sum_k c_k |FFT((x - mean) v_k)|^2 over ntapers
        tapers, mean over segments.  tapers=None: the Slepian sequences windows.dpss(nperseg, nw, ntapers), ntapers=None
        meaning int(2 nw) - 1; or an array [ntapers, nperseg].  weights: 'unity', 'eigen' (the concentration ratios;
        Slepian tapers only) or ntapers non-negative values.  -> a WelchPlan-compatible MtmPlan."""
        return MtmPlan(self, nfft, nperseg, noverlap, nw, ntapers, tapers, weights, detrend, scaling, fs, fftshift,
                       trim_bins, db)

    def mtm_csd_plan(self, nfft, nperseg=None, noverlap=0, nw=4.0, ntapers=None, tapers=None, weights='unity',
                     detrend=DETREND_CONSTANT, scaling=SCALE_DENSITY, fs=1.0, fftshift=False, trim_bins=0, db=False):
        """Two-channel multitaper plan (oth_mtm_csd_plan): mtm_plan's arguments and checks; on top of everything an MtmPlan
        does, csd / csd_exec_dev / csd_partial_dev / csd_scale_dev give Pxx, Pyy, Pxy = mean over segments of
        sum_k c_k conj(X_k) Y_k and Cxy = |Pxy|^2 / (Pxx Pyy) - the three inputs of coherence_detector from one capture
        pair.  -> MtmCsdPlan."""
        return MtmCsdPlan(self, nfft, nperseg, noverlap, nw, ntapers, tapers, weights, detrend, scaling, fs, fftshift,
                          trim_bins, db)

    def chain(self, nfft, window=None, fftshift=True, epilogue=EPI_MAG2, keep_one_in_n=1):
        return Chain(self, nfft, window, fftshift, epilogue, keep_one_in_n)

    def channelizer(self, nchan, decim=None, taps=8, prototype=None):
        """Polyphase channelizer (oth_channelizer): nchan channels (a power of two 64 ... 4096), a new output sample of
        every channel per decim input samples (nchan, nchan / 2 or nchan / 4; nchan // 2 by default), a real prototype of
        taps * nchan taps (1 <= taps <= 16; windows.pfb_prototype(nchan, taps) by default).  -> Channelizer."""
        return Channelizer(self, nchan, decim, taps, prototype)

    # -- cyclic-prefix synchronisation ----------------------------------------------
    def cp_sync(self, x, hyps, rho=1.0, nsamples=None, want_rows=True):
        """Cyclic-prefix symbol timing and carrier offset (oth_cp_sync) of one capture - a host complex64 array, or a device
        pointer with nsamples - at the hypotheses hyps = [(Tu, cp), ...] (1 ... 16 of them; 8 <= Tu <= 16384, 1 <= cp <= Tu).
        -> (gamma, phi, est, nsym): gamma[h] complex64 [Tu + cp] and phi[h] float32 [Tu + cp], the folded correlation and energy
        under the circular cp-window (None, None with want_rows=False); est float32 [nhyp, 4] = theta, eps, rho_hat,
        Lambda[theta] with Lambda = |gamma| - rho phi; nsym uint64 [nhyp] the symbols folded."""
        tu, cp, nhyp, row = cp_sync_args(hyps)
        src, count, dev = _src(x, nsamples)
        gamma = np.zeros((nhyp, row), np.complex64) if want_rows else None
        phi = np.zeros((nhyp, row), np.float32) if want_rows else None
        est = np.empty((nhyp, 4), np.float32)
        nsym = np.zeros(max(nhyp, 1), np.uint64)
        self._call('oth_cp_sync', src, count, dev, nhyp, tu.ctypes.data_as(_ip), cp.ctypes.data_as(_ip), float(rho), row,
                   gamma.ctypes.data_as(_p) if want_rows else None, _fptr(phi) if want_rows else None, _fptr(est),
                   nsym.ctypes.data_as(_u64p))
        if not want_rows:
            return None, None, est, nsym
        ts = tu + cp
        return [gamma[h, :ts[h]] for h in range(nhyp)], [phi[h, :ts[h]] for h in range(nhyp)], est, nsym

    def cp_sync_dev(self, iq_dev, nsamples, hyps, est_dev, gamma_dev=0, phi_dev=0, row_stride=None, rho=1.0, nstreams=1, stride=None):
        """The same on device-resident streams with device outputs (oth_cp_sync_dev), asynchronous on the context's stream:
        nstreams streams every `stride` samples (the rows of Channelizer.push_dev as they are), est_dev float32
        [nstreams][nhyp][4], gamma_dev complex64 and phi_dev float32 [nstreams][nhyp][row_stride] (0: left out; row_stride
        defaults to the largest Tu + cp; the columns behind a hypothesis' Tu + cp are not written).  -> nsym uint64 [nhyp]."""
        tu, cp, nhyp, row = cp_sync_args(hyps)
        nsym = np.zeros(max(nhyp, 1), np.uint64)
        self._call('oth_cp_sync_dev', iq_dev, int(nsamples), int(nstreams), int(nsamples if stride is None else stride), nhyp,
                   tu.ctypes.data_as(_ip), cp.ctypes.data_as(_ip), float(rho), int(row if row_stride is None else row_stride),
                   gamma_dev, phi_dev, est_dev, nsym.ctypes.data_as(_u64p))
        return nsym

    # -- small ops --------------------------------------------------------------
    def rows_group_mean(self, rows, group):
        rows = np.ascontiguousarray(rows, np.float32)
        nrows, nfft = rows.shape
        out = np.empty((nrows // group, nfft), np.float32)
        self._call('oth_rows_group_mean', _fptr(rows), nrows, nfft, group, _fptr(out))
        return out

    def channel_power(self, psd, srch_bins, lo, hi, want_movavg=False):
        psd = np.ascontiguousarray(psd, np.float32)
        lo = np.ascontiguousarray(lo, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        out = np.empty(len(lo), np.float32)
        ma = np.empty(len(psd), np.float32) if want_movavg else None
        self._call('oth_channel_power', _fptr(psd), len(psd), float(srch_bins), len(lo), lo.ctypes.data_as(_ip),
                   hi.ctypes.data_as(_ip), _fptr(out), _fptr(ma) if want_movavg else None)
        return (out, ma) if want_movavg else out

    def bin_threshold(self, psd_rows, srch_bins, thr_leveler):
        """-> (mask uint8[nrows][nfft], noise float32[nrows]) for PSD rows (2-D) or one row (1-D)."""
        rows = np.ascontiguousarray(np.atleast_2d(psd_rows), np.float32)
        nrows, nfft = rows.shape
        mask = np.empty((nrows, nfft), np.uint8)
        noise = np.empty(nrows, np.float32)
        self._call('oth_bin_threshold', _fptr(rows), nrows, nfft, float(srch_bins), float(thr_leveler),
                   mask.ctypes.data_as(_ubp), _fptr(noise))
        return mask, noise

    def scan_decide_dev(self, rows_dptr, nrows, nfft, srch_bins, thr_leveler, lo=(), hi=(), want_mask=True):
        """Decision stage on device-resident PSD rows -> (mask uint8[nrows][nfft] or None, noise[nrows],
        power[nrows][nch])."""
        lo = np.ascontiguousarray(lo, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        nch = len(lo)
        mask = np.empty((nrows, nfft), np.uint8) if want_mask else None
        noise = np.empty(nrows, np.float32)
        power = np.empty((nrows, nch), np.float32)
        self._call('oth_scan_decide_dev', rows_dptr, int(nrows), int(nfft), float(srch_bins), float(thr_leveler), nch,
                   lo.ctypes.data_as(_ip) if nch else None, hi.ctypes.data_as(_ip) if nch else None,
                   mask.ctypes.data_as(_ubp) if want_mask else None, _fptr(noise), _fptr(power) if nch else None)
        return mask, noise, power

    def scan_decide_dev_out(self, rows_dptr, nrows, nfft, srch_bins, thr_leveler, lo, hi, noise_dptr, power_dptr,
                            mask_dptr=0):
        """The same stage with device outputs (asynchronous): noise[nrows], power[nrows][len(lo)], optional mask."""
        lo = np.ascontiguousarray(lo, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        nch = len(lo)
        self._call('oth_scan_decide_dev_out', rows_dptr, int(nrows), int(nfft), float(srch_bins), float(thr_leveler), nch,
                   lo.ctypes.data_as(_ip) if nch else None, hi.ctypes.data_as(_ip) if nch else None, mask_dptr, noise_dptr,
                   power_dptr if nch else None)

    def xcorr(self, a, b, length):
        a, b = _c64(a)[:length], _c64(b)[:length]
        out = np.empty(length - length // 2, np.float32)
        self._call('oth_xcorr', a.ctypes.data_as(_p), len(a), b.ctypes.data_as(_p), len(b), int(length), _fptr(out))
        return out

    def fac(self, data, length):
        a = _c64(data)[:length]
        out = np.empty(length - length // 2, np.float32)
        self._call('oth_fac', a.ctypes.data_as(_p), len(a), int(length), _fptr(out))
        return out


def average_code(average):
    """'mean' / 'median' / AVERAGE_* -> AVERAGE_*; anything else is a ValueError."""
    codes = {'mean': AVERAGE_MEAN, 'median': AVERAGE_MEDIAN}
    if isinstance(average, str):
        if average not in codes:
            raise ValueError("average must be 'mean' or 'median', not %r" % (average,))
        return codes[average]
    if average not in (AVERAGE_MEAN, AVERAGE_MEDIAN):
        raise ValueError('unknown average code %r' % (average,))
    return int(average)


class WelchPlan(_Handle):
    def __init__(self, ctx, nfft, nperseg, noverlap, window, detrend, scaling, fs, fftshift, trim_bins, db, kernel):
        self.ctx = ctx
        # exec_async() tickets not collected yet, and the last one issued; poll() / wait() may run on other threads
        self._tickets, self._last_ticket, self._tickets_lock = set(), 0, threading.Lock()
        nperseg = int(nfft if nperseg is None else nperseg)
        noverlap = int(nperseg // 2 if noverlap is None else noverlap)
        self.nfft, self.nperseg, self.noverlap = int(nfft), nperseg, noverlap
        self.step = nperseg - noverlap
        w = None
        if window is not None:
            w = np.ascontiguousarray(window, np.float32)
            if w.shape != (nperseg,):
                raise ValueError('window must have nperseg=%d entries' % nperseg)
        h = C.c_void_p()
        ctx._call('oth_welch_plan', int(nfft), nperseg, noverlap, _fptr(w) if w is not None else None, int(detrend),
                  int(scaling), float(fs), 1 if fftshift else 0, int(trim_bins), C.byref(h))
        self._created(h, db)
        if kernel != KERNEL_AUTO:
            self._call('oth_plan_set_kernel', int(kernel))

    def _created(self, h, db):
        """the tail of a plan's constructor: the new handle, its output length, dB output where asked for"""
        self.h = h
        n = C.c_int()
        self._call('oth_plan_out_len', C.byref(n))
        self.out_len = n.value
        if db:
            self._call('oth_plan_set_output_db', 1)

    def close(self):
        if getattr(self, 'h', None) and getattr(self.ctx, 'h', None):
            self.ctx.lib.oth_plan_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, k, j):
        """The output rows of a statistic's host form that takes k of them, the first j asked for -> (j float32 rows of
        out_len, k pointers: those rows, then NULL for the rows left out)"""
        rows = [np.empty(self.out_len, np.float32) for _ in range(j)]
        return rows, [_fptr(r) for r in rows] + [None] * (k - j)

    def set_kernel(self, which):
        self._call('oth_plan_set_kernel', int(which))

    def set_tuning(self, variant=None, sched=-1, chunk=0, tail=0):
        """A/B tools and the parity suite: pick a build of the 4096-point kernel ('dpp', 'pipe', 'ws'), override the
        schedule, set the segments per chunk / tail chunk.  Defaults restore the library's choices."""
        v = variant.encode() if variant else None
        self._call('oth_plan_set_tuning', v, int(sched), int(chunk), int(tail))

    def set_schedule(self, which):
        self._call('oth_plan_set_schedule', int(which))

    def set_hostwait(self, sync):
        """True: exec() / wait() sleep in hipStreamSynchronize instead of polling the completion word (low CPU)."""
        self._call('oth_plan_set_hostwait', HOSTWAIT_SYNC if sync else HOSTWAIT_POLL)

    def nseg(self, nsamples):
        return (nsamples - self.noverlap) // self.step if nsamples >= self.nperseg else 0

    average = AVERAGE_MEAN      # (class default: plans start with the mean)

    def set_average(self, average):
        """'mean' / 'median' (or AVERAGE_*): how exec / exec_async / exec_dev average the segments' periodograms.  The
        median refuses the partial / scale / accumulate / csd calls (HipError OTH_ERR_UNSUPPORTED)."""
        code = average_code(average)
        self._call('oth_plan_set_average', code)
        self.average = code

    def segments(self, x):
        """x: host complex64 array -> float32 [nseg, out_len]: one periodogram row per segment with the plan's scaling,
        fftshift, trim and dB (scipy.signal.spectrogram(mode='psd', return_onesided=False) with the axes swapped)."""
        x = _c64(x)
        nseg = self.nseg(len(x))
        if nseg < 1:
            raise ValueError('input shorter than nperseg')
        xd = self.ctx.alloc(x.nbytes)
        try:
            rows = self.ctx.alloc(4 * nseg * self.out_len)
            try:
                self.ctx.h2d(xd, x)
                self.segments_dev(xd, len(x), rows, nseg)
                return self.ctx.d2h(rows, (nseg, self.out_len), np.float32)      # (stream-ordered, then synchronised)
            finally:
                self.ctx.free(rows)
        finally:
            self.ctx.free(xd)

    def segments_dev(self, dptr, nsamples, rows_dptr, capacity):
        """Asynchronous: device in, device out [nseg][out_len] float32 (capacity >= nseg rows).  -> nseg"""
        return self._count('oth_welch_segments_dev', dptr, int(nsamples), rows_dptr, int(capacity))

    def sk(self, x, return_psd=False, nsamples=None):
        """Spectral kurtosis (oth_welch_sk) of one capture: per bin SK = (M + 1) / (M - 1) (M S2 / S1^2 - 1) over the M
        segments' periodograms - 1 for Gaussian noise at any level, towards 0 for a steady line, well above 1 for a signal
        present in under half of the segments.  x: host complex64 array, or a device pointer when nsamples is given.
        -> SK (float32, out_len bins, the plan's fftshift and trim; never dB), or with return_psd (SK, PSD): the row exec()
        gives for the same input.  Sets last_nseg (M).  Needs at least two segments and a mean-averaging Welch plan of a
        power-of-two length 64 ... 16384 (HipError otherwise)."""
        rows, ptrs = self._rows(2, 2 if return_psd else 1)
        src, count, dev = _src(x, nsamples)
        self.last_nseg = self._count('oth_welch_sk', src, count, dev, *ptrs)
        return tuple(rows) if return_psd else rows[0]

    def sk_dev(self, iq_dev, nsamples, nstreams, stride, sk_dev, psd_dev=None):
        """Asynchronous: device in, device out - [nstreams][out_len] float32 at sk_dev and, where given, psd_dev.
        -> segments per stream (also last_nseg)."""
        self.last_nseg = self._count('oth_welch_sk_dev', iq_dev, int(nsamples), int(nstreams), int(stride), sk_dev, psd_dev)
        return self.last_nseg

    ncycles = 0      # (class default: no cycle frequencies until set_cycles)

    def set_cycles(self, alphas):
        """The cycle frequencies of cyclic / cyclic_dev (oth_welch_set_cycles): 1 ... 64 values in cycles per sample, each
        finite with |alpha| <= 0.5, as float64 - a capture of 2^24 samples resolves alpha to 6e-8, below float32's spacing.
        Replaces an earlier set; no other call of the plan is affected.  A multitaper plan, a median-averaging plan and a
        length that is not a power of two 64 ... 16384 raise HipError (OTH_ERR_UNSUPPORTED)."""
        a = np.ascontiguousarray(np.atleast_1d(alphas), np.float64)
        if a.ndim != 1:
            raise ValueError('alphas must be a sequence of cycle frequencies')
        self._call('oth_welch_set_cycles', len(a), a.ctypes.data_as(_dp))
        self.ncycles = len(a)

    def cyclic(self, x, return_psd=False, nsamples=None):
        """Cyclic spectrum and cyclic coherence (oth_welch_cyclic) of one capture at the A cycle frequencies of set_cycles:
        with X_s the plan's windowed transform of segment s and U_s,a the same at frequency f + alpha_a (global time origin),
        scf_a = scale mean_s U_s,a conj(X_s), an estimate of E[X(f + alpha) X*(f)], and coh_a = |sum U conj(X)|^2 /
        (sum |U|^2 sum |X|^2) in [0, 1]: 1 / M for stationary noise of any level or colour, well above for a signal
        that is cyclostationary at alpha_a (CP-OFDM at k / (Tu + Tcp)).  x: host complex64 array, or a device pointer when
        nsamples is given.  -> (scf complex64 [A, out_len], coh float32 [A, out_len]) with the plan's fftshift and trim, and
        with return_psd the row exec() gives for the same input (dB applies to it alone).  Sets last_nseg (M)."""
        A, m = int(self.ncycles), self.out_len
        scf, coh = np.empty((max(A, 1), m), np.complex64), np.empty((max(A, 1), m), np.float32)
        psd = np.empty(m, np.float32) if return_psd else None
        src, count, dev = _src(x, nsamples)
        self.last_nseg = self._count('oth_welch_cyclic', src, count, dev, scf.ctypes.data_as(_f), _fptr(coh),
                                     _fptr(psd) if return_psd else None)
        return (scf, coh, psd) if return_psd else (scf, coh)

    def cyclic_dev(self, iq_dev, nsamples, nstreams, stride, coh_dev, scf_dev=None, psd_dev=None):
        """Asynchronous: device in, device out - [nstreams][A][out_len] float32 at coh_dev and, where given,
        [nstreams][A][out_len] re, im pairs at scf_dev and [nstreams][out_len] at psd_dev.
        -> segments per stream (also last_nseg)."""
        self.last_nseg = self._count('oth_welch_cyclic_dev', iq_dev, int(nsamples), int(nstreams), int(stride), scf_dev, coh_dev,
                                     psd_dev)
        return self.last_nseg

    nlags = 0      # (class default: no lags until set_lags)

    def set_lags(self, lags):
        """The lags of caf / caf_dev (oth_welch_set_lags): 1 ... 64 integers in samples, each 0 ... 65535.  Replaces an
        earlier set; no other call of the plan is affected.  A multitaper plan, a median-averaging plan and a length that is
        not a power of two 64 ... 16384 raise HipError (OTH_ERR_UNSUPPORTED)."""
        a = np.atleast_1d(np.asarray(lags))
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError('lags must be a sequence of integer lags in samples')
        a = np.ascontiguousarray(np.clip(a.astype(np.int64), -1, 1 << 30), np.intc)      # (out of range stays out of range)
        self._call('oth_welch_set_lags', len(a), a.ctypes.data_as(_ip))
        self.nlags = len(a)

    def caf(self, x, return_r=False, nsamples=None):
        """Cyclic autocorrelation (oth_welch_caf) of one capture at the L lags of set_lags, as the plan's Welch PSD of the
        lag product z_l[n] = x[n + tau_l] conj(x[n]): row l, bin q is the power of z_l at cycle frequency alpha = q / nfft
        cycles per sample (the upper half of a row holds negative alpha, as for a PSD).  A CP-OFDM signal shows lines at
        k / (Tu + Tcp) in the row of tau = Tu; stationary noise shows a flat floor at every lag.  The segments are counted
        on nsamples - max(lags) samples.  x: host complex64 array, or a device pointer when nsamples is given.
        -> caf float32 [L, out_len] with the plan's scaling, fftshift, trim and dB, and with return_r also r complex64 [L]:
        the mean of z_l over all segments, the autocorrelation estimate R(tau_l), never scaled.  Sets last_nseg (M)."""
        L, m = int(self.nlags), self.out_len
        caf = np.empty((max(L, 1), m), np.float32)
        r = np.empty(max(L, 1), np.complex64) if return_r else None
        src, count, dev = _src(x, nsamples)
        self.last_nseg = self._count('oth_welch_caf', src, count, dev, _fptr(caf), r.ctypes.data_as(_f) if return_r else None)
        return (caf, r) if return_r else caf

    def caf_dev(self, iq_dev, nsamples, nstreams, stride, caf_dev, r_dev=None):
        """Asynchronous: device in, device out - [nstreams][L][out_len] float32 at caf_dev and, where given, [nstreams][L]
        re, im pairs at r_dev.  -> segments per stream (also last_nseg)."""
        self.last_nseg = self._count('oth_welch_caf_dev', iq_dev, int(nsamples), int(nstreams), int(stride), caf_dev, r_dev)
        return self.last_nseg

    ntaps = 0      # (class default: no prototype until set_prototype)

    def set_prototype(self, h, ntaps=None):
        """The prototype of pfb / pfb_dev (oth_welch_set_prototype): ntaps * nfft real taps, 2 <= ntaps <= 16 taps per
        branch (ntaps from len(h) / nfft when it is left out; windows.pfb_prototype gives a Kaiser-windowed sinc).  Replaces
        an earlier prototype; no other call of the plan is affected.  A multitaper plan, a median-averaging plan, a length
        that is not a power of two 64 ... 16384 and a plan with nperseg != nfft raise HipError (OTH_ERR_UNSUPPORTED)."""
        a = np.ascontiguousarray(np.asarray(h, np.float64).ravel(), np.float32)
        if ntaps is None:
            if len(a) == 0 or len(a) % self.nfft:
                raise ValueError('the prototype holds ntaps * nfft taps: %d is no multiple of %d' % (len(a), self.nfft))
            ntaps = len(a) // self.nfft
        elif 1 <= int(ntaps) and len(a) != int(ntaps) * self.nfft:
            raise ValueError('the prototype holds ntaps * nfft = %d taps, not %d' % (int(ntaps) * self.nfft, len(a)))
        self._call('oth_welch_set_prototype', int(ntaps), _fptr(a))
        self.ntaps = int(ntaps)

    def pfb(self, x, nsamples=None):
        """Polyphase filter-bank (WOLA) PSD (oth_welch_pfb) of one capture under the prototype of set_prototype: every
        frame of ntaps * nfft samples, one every nfft - noverlap samples, is weighted by the prototype, folded onto nfft
        points and transformed; the row is the mean of |X|^2 over the M = (n - ntaps nfft) / step + 1 frames - every
        ntaps-th bin of a Welch PSD of ntaps * nfft points with the prototype as its window, so a bin has a flat top and a
        stop band one bin away.  x: host complex64 array, or a device pointer when nsamples is given.
        -> float32 [out_len] with the plan's scaling (the prototype in the window's place), fftshift, trim and dB.  Sets
        last_nseg (M)."""
        out = np.empty(self.out_len, np.float32)
        src, count, dev = _src(x, nsamples)
        self.last_nseg = self._count('oth_welch_pfb', src, count, dev, _fptr(out))
        return out

    def pfb_dev(self, iq_dev, nsamples, nstreams, stride, out_dev):
        """Asynchronous: device in, device out - [nstreams][out_len] float32 at out_dev.  -> frames per stream (also
        last_nseg)."""
        self.last_nseg = self._count('oth_welch_pfb_dev', iq_dev, int(nsamples), int(nstreams), int(stride), out_dev)
        return self.last_nseg

    def matrix(self, x, return_gcoh=True, nsamples=None):
        """Spectral matrix and generalized coherence (oth_welch_matrix) of C coherent channels, 2 <= C <= 8: with X_s,a the
        plan's windowed transform of segment s of channel a, S[a][b] = scale mean_s conj(X_s,a) X_s,b - scipy.signal.csd(x_a,
        x_b) with the plan's parameters, the diagonal scipy.signal.welch - and gcoh = 1 - det G, G_ab = S_ab / sqrt(S_aa S_bb),
        in [0, 1]: the Hadamard ratio, independent of every channel's gain and noise floor, near 1 - prod_k (M - k) / M for
        independent noise and near 1 where the channels share a signal.  x: host complex64 array (C, n), or a device pointer
        to [C][nsamples] when nsamples is given as (C, nsamples).  -> (S complex64 [C, C, out_len], always linear, with
        S[b][a] = conj(S[a][b]) and the plan's fftshift and trim, gcoh float32 [out_len]), or S alone with
        return_gcoh=False.  A bin where a channel holds no power reads 0 in that channel's rows and in gcoh.  Sets
        last_nseg (M); with M < C the matrix is singular and gcoh reads 1."""
        src, count, nchan, dev = _channels(x, nsamples)
        m, pairs = self.out_len, nchan * (nchan + 1) // 2
        packed = np.empty((pairs, m), np.complex64)
        gcoh = np.empty(m, np.float32) if return_gcoh else None
        self.last_nseg = self._count('oth_welch_matrix', src, count, nchan, dev, packed.ctypes.data_as(_f),
                                     _fptr(gcoh) if return_gcoh else None)
        S = unpack_matrix(packed, nchan)
        return (S, gcoh) if return_gcoh else S

    def matrix_dev(self, iq_dev, nsamples, nchan, stride, s_dev=None, gcoh_dev=None):
        """Asynchronous: device in, device out - the packed upper triangle [C (C + 1) / 2][out_len] re, im pairs at s_dev
        (pairs (0,0), (0,1), ..., (0,C-1), (1,1), ...: unpack_matrix) and [out_len] float32 at gcoh_dev; either may be left
        out, not both.  stride: samples between channels.  -> segments per channel (also last_nseg)."""
        self.last_nseg = self._count('oth_welch_matrix_dev', iq_dev, int(nsamples), int(nchan), int(stride), s_dev, gcoh_dev)
        return self.last_nseg

    def matrix_eig(self, x, of='S', return_vector=True, nsamples=None):
        """Eigenvalues and principal eigenvector per bin (oth_welch_matrix_eig) of the spectral matrix S of matrix()
        (of='S' or EIG_OF_S) or of its coherence matrix G_ab = S_ab / sqrt(S_aa S_bb) (of='G' or EIG_OF_G: unit diagonal,
        unchanged by a gain per channel).  x as in matrix(): host complex64 array (C, n), or a device pointer to
        [C][nsamples] when nsamples is given as (C, nsamples).  -> (eig float32 [C, out_len], row k the k-th largest
        eigenvalue, always linear, with the plan's fftshift and trim, vec complex64 [C, out_len], the unit eigenvector of
        the largest eigenvalue with component 0 real and >= 0), or eig alone with return_vector=False.  A bin with a silent
        channel reads an exact 0 eigenvalue of S and all ones of G; a non-finite sample reads NaN everywhere.  Sets
        last_nseg (M); with M < C the trailing C - M eigenvalues read 0 up to rounding."""
        src, count, nchan, dev = _channels(x, nsamples)
        m = self.out_len
        eig = np.empty((nchan, m), np.float32)
        vec = np.empty((nchan, m), np.complex64) if return_vector else None
        self.last_nseg = self._count('oth_welch_matrix_eig', src, count, nchan, dev, _eig_of(of), _fptr(eig),
                                     vec.ctypes.data_as(_f) if return_vector else None)
        return (eig, vec) if return_vector else eig

    def matrix_eig_dev(self, iq_dev, nsamples, nchan, stride, of, eig_dev=None, vec_dev=None):
        """Asynchronous: device in, device out - [C][out_len] float32 at eig_dev (the rows descend) and [C][out_len] re, im
        pairs at vec_dev; either may be left out, not both.  of: 'S' / 'G' or EIG_OF_S / EIG_OF_G.  stride: samples between
        channels.  -> segments per channel (also last_nseg)."""
        self.last_nseg = self._count('oth_welch_matrix_eig_dev', iq_dev, int(nsamples), int(nchan), int(stride), _eig_of(of),
                                     eig_dev, vec_dev)
        return self.last_nseg

    ndir = 0      # (class default: no steering table until set_steering)
    DOA_METHODS = ('bartlett', 'capon', 'music')

    def set_steering(self, delays, fc):
        """The steering table of matrix_doa / matrix_doa_dev (oth_welch_set_steering): delays [D, C] in samples, fractional
        or negative as they come, 1 <= D <= 1024 directions of 2 <= C <= 8 channels - channel c of direction d carries
        s(t - delays[d, c]) -, and fc the carrier in cycles per sample (0 for a baseband array).  Replaces an earlier
        table; an empty array clears it."""
        a = np.ascontiguousarray(delays, np.float64)
        if a.size == 0:
            self._call('oth_welch_set_steering', 0, 0, None, float(fc))
            self.ndir = 0
            return
        if a.ndim != 2:
            raise ValueError('delays must be a (D, C) array: a row of C channel delays per direction')
        self._call('oth_welch_set_steering', a.shape[0], a.shape[1], a.ctypes.data_as(_dp), float(fc))
        self.ndir = a.shape[0]

    def matrix_doa(self, x, of='S', nsrc=None, loading=0.0, methods=('bartlett', 'capon', 'music'), nsamples=None):
        """Direction spectra per bin (oth_welch_matrix_doa) over the D directions of set_steering, of the spectral matrix S
        of matrix() (of='S') or of its coherence matrix G (of='G': a gain per channel drops out).  With w the steering
        vector of a direction at a bin, l_i and v_i the eigenvalues (descending) and eigenvectors of the bin's matrix A,
        p_i = |v_i^H w|^2 and delta = loading trace(A) / C:
          'bartlett'  w^H A w / C^2                        the conventional beamformer
          'capon'     1 / w^H (A + delta I)^-1 w           MVDR; 0 in a bin where A + delta I is singular
          'music'     C / sum_{i > nsrc} p_i               nsrc: the dimension of the signal subspace, 1 ... C - 1
        x as in matrix(): host complex64 array (C, n), or a device pointer to [C][nsamples] when nsamples is given as
        (C, nsamples).  -> dict method -> float32 [D, out_len] for the methods asked for, always linear, with the plan's
        fftshift and trim.  A non-finite sample reads NaN everywhere.  Sets last_nseg (M)."""
        methods = (methods,) if isinstance(methods, str) else tuple(methods)
        if not methods or any(m not in self.DOA_METHODS for m in methods):
            raise ValueError("methods must name at least one of 'bartlett', 'capon', 'music'")
        if 'music' in methods and nsrc is None:
            raise ValueError('the MUSIC spectrum needs nsrc, the number of sources')
        src, count, nchan, dev = _channels(x, nsamples)
        rows = {m: np.empty((self.ndir, self.out_len), np.float32) for m in methods}
        self.last_nseg = self._count('oth_welch_matrix_doa', src, count, nchan, dev, _eig_of(of), int(nsrc or 0), float(loading),
                                     *[_fptr(rows[m]) if m in rows else None for m in self.DOA_METHODS])
        return rows

    def matrix_doa_dev(self, iq_dev, nsamples, nchan, stride, of, nsrc, loading, bartlett_dev=None, capon_dev=None, music_dev=None):
        """Asynchronous: device in, device out - [D][out_len] float32 at each of bartlett_dev, capon_dev and music_dev; any may
        be left out, not all three (nsrc is read only with music_dev).  of: 'S' / 'G' or EIG_OF_S / EIG_OF_G.  stride: samples
        between channels.  -> segments per channel (also last_nseg)."""
        self.last_nseg = self._count('oth_welch_matrix_doa_dev', iq_dev, int(nsamples), int(nchan), int(stride), _eig_of(of),
                                     int(nsrc or 0), float(loading), bartlett_dev, capon_dev, music_dev)
        return self.last_nseg

    def _gcc_args(self, band, upsample, maxlag):
        """band=None: every bin; maxlag=None: NI / 2 - 1 (NI = upsample nfft) -> (lo, hi, upsample, maxlag) as integers"""
        lo, hi = (-(self.nfft // 2), self.nfft // 2 - 1) if band is None else (int(band[0]), int(band[1]))
        upsample = int(upsample)
        return lo, hi, upsample, (max(upsample, 1) * self.nfft // 2 - 1 if maxlag is None else int(maxlag))

    def matrix_gcc(self, x, weighting='phat', band=None, upsample=1, maxlag=None, return_rows=True, nsamples=None):
        """Generalized cross-correlation and the delay of every pair of C coherent channels (oth_welch_matrix_gcc),
        2 <= C <= 8: the inverse transform of the weighted sums T_ab of matrix() over a band, R_ab[l] = (1 / Z) sum_k w_k
        T_ab[k] / |T_ab[k]| e^(+j 2 pi k l / NI) with w = 1 ('phat'), |T_ab| / sqrt(T_aa T_bb) ('scot') or |T_ab| ('plain':
        the band's correlation coefficient) and |R| <= 1.  band: (lo, hi) signed bins of the natural transform, both
        inclusive, in -nfft / 2 ... nfft / 2 - 1 (None: all of them); upsample U: 1, 2, 4 or 8 with NI = U nfft <= 16384 -
        lags count 1 / U sample (band-limited interpolation: it removes the parabola's bias at U = 1); maxlag: the rows hold
        the lags -maxlag ... maxlag, 0 <= maxlag <= NI / 2 - 1 (None: the largest).  Channel c carries s(t - tau_c), the
        convention of set_steering: |R_ab| peaks at tau_b - tau_a.  x as in matrix(): host complex64 array (C, n), or a
        device pointer to [C][nsamples] when nsamples is given as (C, nsamples).
        -> (delays float32 [C, C] in samples, delays[a][b] = tau_b - tau_a at the peak of |R_ab| with a parabola through its
        neighbours, antisymmetric; peaks float32 [C, C], |R_ab| at the peak, symmetric, the diagonal 1; phases float32
        [C, C], arg R_ab at the peak in radians, antisymmetric; rows complex64 [C (C - 1) / 2, 2 maxlag + 1], pairs in the
        order of gcc_pairs(C)), or the first three with return_rows=False.  The plan's scaling, fftshift, trim and dB take
        no part.  A pair with a silent channel reads 0 everywhere; a non-finite sample reads NaN in its channel's pairs.
        Sets last_nseg (M)."""
        src, count, nchan, dev = _channels(x, nsamples)
        lo, hi, upsample, maxlag = self._gcc_args(band, upsample, maxlag)
        npairs = nchan * (nchan - 1) // 2
        rows = np.empty((npairs, 2 * max(maxlag, 0) + 1), np.complex64) if return_rows else None
        peak = np.empty((npairs, 3), np.float32)
        self.last_nseg = self._count('oth_welch_matrix_gcc', src, count, nchan, dev, _gcc_weighting(weighting), lo, hi, upsample,
                                     maxlag, rows.ctypes.data_as(_f) if return_rows else None, _fptr(peak))
        delays, peaks, phases = np.zeros((nchan, nchan), np.float32), np.eye(nchan, dtype=np.float32), np.zeros((nchan, nchan), np.float32)
        for (a, b), (tau, top, arg) in zip(gcc_pairs(nchan), peak):
            delays[a, b], delays[b, a] = tau, -tau
            peaks[a, b] = peaks[b, a] = top
            phases[a, b], phases[b, a] = arg, -arg
        return (delays, peaks, phases, rows) if return_rows else (delays, peaks, phases)

    def matrix_gcc_dev(self, iq_dev, nsamples, nchan, stride, weighting='phat', band=None, upsample=1, maxlag=None, gcc_dev=None, peak_dev=None):
        """Asynchronous: device in, device out - [C (C - 1) / 2][2 maxlag + 1] re, im pairs at gcc_dev and [C (C - 1) / 2][3]
        float32 (delay in samples, |R|, arg R at the peak) at peak_dev; either may be left out, not both.  weighting, band,
        upsample and maxlag as in matrix_gcc.  stride: samples between channels.  -> segments per channel (also last_nseg)."""
        lo, hi, upsample, maxlag = self._gcc_args(band, upsample, maxlag)
        self.last_nseg = self._count('oth_welch_matrix_gcc_dev', iq_dev, int(nsamples), int(nchan), int(stride),
                                     _gcc_weighting(weighting), lo, hi, upsample, maxlag, gcc_dev, peak_dev)
        return self.last_nseg

    def last_recipe(self):
        """Diagnostics: 'kernel=... form=... pilot=... sched=... chunk=... W=...' of the last averaging launch."""
        buf = C.create_string_buffer(512)
        self._call('oth__debug_last_recipe', buf, 512)
        return buf.value.decode()

    def _exec(self, x, nsamples):
        """exec (nsamples=None) and exec_device_src"""
        out = np.empty(self.out_len, np.float32)
        src, count, dev = _src(x, nsamples)
        self.last_nseg = self._count('oth_welch_exec', src, count, dev, _fptr(out))
        return out

    def exec(self, x):
        """x: host complex64 array -> float32 PSD of out_len bins."""
        return self._exec(x, None)

    def exec_device_src(self, dptr, nsamples):
        return self._exec(dptr, nsamples)

    def exec_async(self, x, nsamples=None):
        """work() form: enqueue one Welch scan and return a ticket at once.  x: host complex64 array (may be reused as
        soon as the call returns), or a device pointer when nsamples is given."""
        src, count, dev = _src(x, nsamples)
        t = C.c_uint64()
        # direct, not the helper: on the work() path its extra Python call showed (profiles/binding_fold_ab.txt)
        self.ctx.check(self.ctx.lib.oth_welch_exec_async(self.h, src, count, dev, C.byref(t)), 'oth_welch_exec_async')
        with self._tickets_lock:
            self._tickets.add(int(t.value))
            self._last_ticket = int(t.value)
        return int(t.value)

    @property
    def outstanding(self):
        """exec_async() tickets not collected yet (Context.cached_plan never closes a plan that owes one)."""
        with self._tickets_lock:
            return len(self._tickets)

    def next_ticket_slot_free(self):
        """True when the next exec_async() ticket - the one after the last, on a plan that serves exec_async() only -
        delivers into an output slot that holds no uncollected ticket, i.e. it overwrites nothing anybody still waits for."""
        with self._tickets_lock:
            return self._last_ticket + 1 - OUT_RING not in self._tickets

    def _collected(self, ticket):
        with self._tickets_lock:
            self._tickets.discard(int(ticket))

    def poll(self, ticket):
        """-> None while the GPU is still working, else the float32 PSD (last_nseg is set)."""
        out = np.empty(self.out_len, np.float32)
        n, ready = C.c_uint64(), C.c_int()
        # direct, not the helper: on the work() path its extra Python call showed (profiles/binding_fold_ab.txt)
        self.ctx.check(self.ctx.lib.oth_welch_poll(self.h, int(ticket), _fptr(out), C.byref(n), C.byref(ready)), 'oth_welch_poll')
        if not ready.value:
            return None
        self._collected(ticket)
        self.last_nseg = n.value
        return out

    def wait(self, ticket):
        out = np.empty(self.out_len, np.float32)
        n = C.c_uint64()
        try:
            # direct, not the helper: on the work() path its extra Python call showed (profiles/binding_fold_ab.txt)
            self.ctx.check(self.ctx.lib.oth_welch_wait(self.h, int(ticket), _fptr(out), C.byref(n)), 'oth_welch_wait')
        finally:
            self._collected(ticket)
        self.last_nseg = n.value
        return out

    def exec_dev(self, dptr, nsamples, out_dptr, nstreams=1, stream_stride=None):
        """Asynchronous: device in, device out ([nstreams][out_len] float32)."""
        stride = nsamples if stream_stride is None else stream_stride
        return self._count('oth_welch_exec_dev', dptr, nsamples, nstreams, stride, out_dptr)

    def partial_dev(self, dptr, nsamples, sum_dptr):
        return self._count('oth_welch_partial_dev', dptr, nsamples, sum_dptr)

    def scale_dev(self, sum_dptr, nseg_total, out_dptr):
        self._call('oth_welch_scale_dev', sum_dptr, nseg_total, out_dptr)

    def accumulate(self, x):
        x = _c64(x)
        self._call('oth_welch_accumulate', x.ctypes.data_as(_p), len(x))

    def finalize(self):
        out = np.empty(self.out_len, np.float32)
        self.last_nseg = self._count('oth_welch_finalize', _fptr(out))
        return out

    def reset(self):
        self._call('oth_welch_reset')

    def _csd(self, x, y, nsamples):
        """csd (nsamples=None) and csd_device_src"""
        m = self.out_len
        pxx, pyy, cxy = (np.empty(m, np.float32) for _ in range(3))
        pxy = np.empty(2 * m, np.float32)
        sx, sy, count, dev = _src2(x, y, nsamples)
        self.last_nseg = self._count('oth_csd_exec', sx, sy, count, dev, _fptr(pxx), _fptr(pyy), _fptr(pxy), _fptr(cxy))
        return pxx, pyy, pxy.view(np.complex64), cxy

    def csd(self, x, y):
        """-> pxx, pyy, pxy (complex64), cxy for host inputs."""
        return self._csd(x, y, None)

    def csd_device_src(self, dx, dy, nsamples):
        """-> pxx, pyy, pxy (complex64), cxy for device inputs."""
        return self._csd(dx, dy, nsamples)

    def csd_exec_dev(self, dx, dy, nsamples, pxx=0, pyy=0, pxy=0, cxy=0):
        """Asynchronous: device in, device out (any output pointer may be 0)."""
        return self._count('oth_csd_exec_dev', dx, dy, nsamples, pxx, pyy, pxy, cxy)

    def csd_partial_dev(self, dx, dy, nsamples, sums_dptr):
        """Raw sums [sum|X|^2 | sum|Y|^2 | sum conj(X)Y re,im] (4 * nfft floats, natural order) of this time chunk."""
        return self._count('oth_csd_partial_dev', dx, dy, nsamples, sums_dptr)

    def csd_scale_dev(self, sums_dptr, nseg_total, pxx=0, pyy=0, pxy=0, cxy=0):
        self._call('oth_csd_scale_dev', sums_dptr, int(nseg_total), pxx, pyy, pxy, cxy)


def mtm_weights(weights, ntapers, slepian=True):
    """'unity' -> None (uniform), 'eigen' -> 'eigen' (the plan's concentration ratios: its own Slepian tapers only), an
    array -> float32 [ntapers]; anything the library would refuse is a ValueError here, before it is called."""
    if isinstance(weights, str):
        if weights == 'unity':
            return None
        if weights != 'eigen':
            raise ValueError("weights must be 'unity', 'eigen' or an array, not %r" % (weights,))
        if not slepian:
            raise ValueError("weights='eigen' needs the plan's own Slepian tapers (tapers=None)")
        return 'eigen'
    w = np.asarray(weights, np.float64)
    if w.shape != (ntapers,):
        raise ValueError('weights must have ntapers=%d entries' % ntapers)
    w32 = np.ascontiguousarray(w, np.float32)
    if not np.all(np.isfinite(w32)) or np.any(w < 0.0) or not w32.sum() > 0.0:
        raise ValueError('weights must be finite, non-negative and have a positive sum')
    return w32


class MtmPlan(WelchPlan):
    """A WelchPlan whose averaging launch is the multitaper kernel: exec / exec_async / poll / wait / exec_dev /
    partial_dev / scale_dev / accumulate / finalize / reset as WelchPlan's; the median average, the per-segment rows,
    the cross spectrum, KERNEL_TUNED and build variants raise HipError (OTH_ERR_UNSUPPORTED).  ftest / ftest_dev: Thomson's
    harmonic F-test on the same tapers.  adaptive / adaptive_dev: Thomson's adaptive weighting and its degrees of freedom
    (the plan's own Slepian tapers bring their concentration ratios; set_ratios() gives them for user tapers)."""

    _CONSTRUCTOR = 'oth_mtm_plan'

    def __init__(self, ctx, nfft, nperseg, noverlap, nw, ntapers, tapers, weights, detrend, scaling, fs, fftshift,
                 trim_bins, db):
        from . import windows
        self.ctx = ctx
        self._tickets, self._last_ticket, self._tickets_lock = set(), 0, threading.Lock()
        nperseg = int(nfft if nperseg is None else nperseg)
        noverlap = int(noverlap)
        self.nfft, self.nperseg, self.noverlap = int(nfft), nperseg, noverlap
        self.step = nperseg - noverlap
        ratios, slepian = None, tapers is None
        if slepian:
            ntapers = int(2 * nw) - 1 if ntapers is None else int(ntapers)
            if ntapers < 1:
                raise ValueError('ntapers must be at least 1 (nw=%r gives int(2 nw) - 1 = %d)' % (nw, ntapers))
        else:
            tapers = np.ascontiguousarray(tapers, np.float32)
            if tapers.ndim != 2 or tapers.shape[1] != nperseg or (ntapers is not None and tapers.shape[0] != int(ntapers)):
                raise ValueError('tapers must have shape [ntapers, nperseg=%d]' % nperseg)
            ntapers = tapers.shape[0]
        w = mtm_weights(weights, ntapers, slepian)
        if slepian:
            tapers, ratios = windows.dpss(nperseg, nw, ntapers, return_ratios=True)
        if isinstance(w, str):
            w = np.ascontiguousarray(ratios, np.float32)
        t = np.ascontiguousarray(tapers, np.float32)
        self.ntapers = ntapers
        self.tapers, self.ratios = t, ratios
        h = C.c_void_p()
        ctx._call(self._CONSTRUCTOR, int(nfft), nperseg, noverlap, self.ntapers, _fptr(t), _fptr(w) if w is not None else None,
                  int(detrend), int(scaling), float(fs), 1 if fftshift else 0, int(trim_bins), C.byref(h))
        self._created(h, db)
        if slepian:      # (the computed ratio of a taper can come out an ulp past 1, or not above 0 far beyond 2 nw tapers)
            self.set_ratios(np.clip(ratios, np.finfo(np.float64).tiny, 1.0))
            self.ratios = ratios

    def set_ratios(self, ratios):
        """The tapers' concentration ratios lambda_k (oth_mtm_set_ratios), each in (0, 1], as float64 - the adaptive estimate
        needs 1 - lambda_k, which a float32 lambda_0 does not hold.  Replaces an earlier set; no other call reads them."""
        r = np.ascontiguousarray(ratios, np.float64)
        if r.shape != (self.ntapers,):
            raise ValueError('ratios must have ntapers=%d entries' % self.ntapers)
        self._call('oth_mtm_set_ratios', r.ctypes.data_as(_dp))
        self.ratios = r

    def adaptive(self, x, iters=4, return_dof=False, nsamples=None):
        """Thomson's adaptive-weight estimate (oth_mtm_adaptive) of one capture: per segment and bin the eigenspectra are
        combined with weights lambda_k b_k^2, b_k = S / (lambda_k S + (1 - lambda_k) sigma^2), S updated `iters` times from
        (P_0 + P_1) / 2 - a taper leaves a bin as far as its leakage would dominate there, so an empty band next to a strong
        one is not lifted as it is with fixed weights.  x: host complex64 array, or a device pointer when nsamples is given.
        -> PSD (float32, out_len bins, the plan's scaling, fftshift, trim and dB), or with return_dof (PSD, dof): the per-bin
        equivalent degrees of freedom 2 (sum w)^2 / sum w^2, mean over the segments, between 2 and 2 K, always linear.
        Sets last_nseg.  The plan's weights take no part."""
        rows, ptrs = self._rows(2, 2 if return_dof else 1)
        src, count, dev = _src(x, nsamples)
        self.last_nseg = self._count('oth_mtm_adaptive', src, count, dev, int(iters), *ptrs)
        return tuple(rows) if return_dof else rows[0]

    def adaptive_dev(self, iq_dev, nsamples, nstreams, stride, psd_dev, dof_dev=None, iters=4):
        """Asynchronous: device in, device out - [nstreams][out_len] float32 at psd_dev and, where given, dof_dev.
        -> segments per stream (also last_nseg)."""
        self.last_nseg = self._count('oth_mtm_adaptive_dev', iq_dev, int(nsamples), int(nstreams), int(stride), int(iters), psd_dev,
                                     dof_dev)
        return self.last_nseg

    def ftest(self, x, return_rows=False, nsamples=None):
        """Thomson's harmonic F-test (oth_mtm_ftest) of one capture: per bin F = (K - 1) sum_s num_s / sum_s den_s, large
        where a coherent line sits at the bin whatever the background.  x: host complex64 array, or a device pointer when
        nsamples is given.  -> F (float32, out_len bins, the plan's fftshift and trim; always linear), or with return_rows
        (F, line, resid): the line's power and the background with the line removed.  Sets last_nseg (see dof)."""
        rows, ptrs = self._rows(3, 3 if return_rows else 1)
        src, count, dev = _src(x, nsamples)
        self.last_nseg = self._count('oth_mtm_ftest', src, count, dev, *ptrs)
        return tuple(rows) if return_rows else rows[0]

    def ftest_dev(self, iq_dev, nsamples, nstreams, stride, f_dev, line_dev=None, resid_dev=None):
        """Asynchronous: device in, device out - [nstreams][out_len] float32 at f_dev and, where given, line_dev and
        resid_dev.  -> segments per stream (also last_nseg)."""
        self.last_nseg = self._count('oth_mtm_ftest_dev', iq_dev, int(nsamples), int(nstreams), int(stride), f_dev, line_dev,
                                     resid_dev)
        return self.last_nseg

    def jackknife(self, x, return_psd=False, nsamples=None):
        """Jackknife (oth_mtm_jackknife) of one capture over its M = ntapers * nseg (segment, taper) items: per bin the
        standard deviation of ln PSD, in natural-log units - the interval at Student-t quantile q (M - 1 degrees of freedom)
        is psd * exp(-+ q * lnsd).  x: host complex64 array, or a device pointer when nsamples is given.  -> lnsd (float32,
        out_len bins, the plan's fftshift and trim; never dB, never scaled), or with return_psd (lnsd, PSD): the row exec()
        gives for the same input.  Sets last_nseg.  Needs equal weights and M >= 2 (HipError otherwise)."""
        rows, ptrs = self._rows(2, 2 if return_psd else 1)
        src, count, dev = _src(x, nsamples)
        self.last_nseg = self._count('oth_mtm_jackknife', src, count, dev, *ptrs)
        return tuple(rows) if return_psd else rows[0]

    def jackknife_dev(self, iq_dev, nsamples, nstreams, stride, lnsd_dev, psd_dev=None):
        """Asynchronous: device in, device out - [nstreams][out_len] float32 at lnsd_dev and, where given, psd_dev.
        -> segments per stream (also last_nseg)."""
        self.last_nseg = self._count('oth_mtm_jackknife_dev', iq_dev, int(nsamples), int(nstreams), int(stride), lnsd_dev, psd_dev)
        return self.last_nseg

    @property
    def dof(self):
        """Degrees of freedom (2 nseg, 2 nseg (K - 1)) of the F distribution the last call's bins follow without a line."""
        nseg = int(getattr(self, 'last_nseg', 0))
        return 2 * nseg, 2 * nseg * (self.ntapers - 1)


class MtmCsdPlan(MtmPlan):
    """An MtmPlan on which the inherited two-channel calls - csd, csd_device_src, csd_exec_dev, csd_partial_dev,
    csd_scale_dev - run the two-channel taper loop (oth_mtm_csd_plan) instead of raising."""

    _CONSTRUCTOR = 'oth_mtm_csd_plan'

    def csd_jackknife(self, x, y, nsamples=None):
        """Jackknife (oth_mtm_csd_jackknife) of a pair of captures over their M = ntapers * nseg items -> (cxy, zsd, lnsd_x,
        lnsd_y), float32 rows of out_len bins with the plan's fftshift and trim: the coherence csd() gives, the standard
        deviation of z = atanh(sqrt(cxy)) - the interval at Student-t quantile q (M - 1 degrees of freedom) is
        tanh(max(0, z -+ q * zsd)) ** 2 - and of each channel's ln PSD.  x, y: host complex64 arrays, or device pointers
        when nsamples is given.  Sets last_nseg.  Needs equal weights and M >= 3 (HipError otherwise)."""
        rows, ptrs = self._rows(4, 4)
        sx, sy, count, dev = _src2(x, y, nsamples)
        self.last_nseg = self._count('oth_mtm_csd_jackknife', sx, sy, count, dev, *ptrs)
        return tuple(rows)

    def csd_jackknife_dev(self, dx, dy, nsamples, zsd_dev, cxy_dev=None, lnsdx_dev=None, lnsdy_dev=None):
        """Asynchronous: device in, device out - out_len float32 at zsd_dev and, where given, cxy_dev, lnsdx_dev and
        lnsdy_dev.  -> segments (also last_nseg)."""
        self.last_nseg = self._count('oth_mtm_csd_jackknife_dev', dx, dy, int(nsamples), cxy_dev, zsd_dev, lnsdx_dev, lnsdy_dev)
        return self.last_nseg


class Chain(_Handle):
    """stream_to_vector -> keep_one_in_n -> fft_vcc -> |.|/|.|^2 [-> IIR -> log] with GNU Radio's
    streaming state kept on the device (oth_chain)."""

    def __init__(self, ctx, nfft, window, fftshift, epilogue, keep_one_in_n):
        self.ctx = ctx
        self.nfft = int(nfft)
        w = None
        if window is not None and len(window):
            w = np.ascontiguousarray(window, np.float32)
            if w.shape != (self.nfft,):
                raise ValueError('window must have nfft entries')
        h = C.c_void_p()
        ctx._call('oth_chain_create', self.nfft, _fptr(w) if w is not None else None, 1 if fftshift else 0, int(epilogue),
                  int(keep_one_in_n), C.byref(h))
        self.h = h

    def close(self):
        if getattr(self, 'h', None) and getattr(self.ctx, 'h', None):
            self.ctx.lib.oth_chain_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_keep_one_in_n(self, n):
        self._call('oth_chain_set_keep_one_in_n', int(n))

    def set_iir_log(self, alpha, k_db):
        self._call('oth_chain_set_iir_log', float(alpha), float(k_db))

    def set_kernel(self, which):
        self._call('oth_chain_set_kernel', int(which))

    def set_peak_hold(self, on):
        self._call('oth_chain_set_peak_hold', 1 if on else 0)

    def reset(self):
        self._call('oth_chain_reset')

    def push(self, x, max_rows=None):
        """Feed samples; returns (rows, nrows_produced).  rows holds the LAST min(nrows, max_rows) rows."""
        x = _c64(x)
        cap = (len(x) // self.nfft + 2) if max_rows is None else int(max_rows)
        rows = np.empty((max(cap, 1), self.nfft), np.float32)
        n = self._count('oth_chain_push', x.ctypes.data_as(_p), len(x), 0, _fptr(rows), cap)
        return rows[:min(n, cap)], n

    def push_dev(self, dptr, nsamples, rows_dptr=0, capacity=0):
        """Asynchronous: device-resident samples in, the last `capacity` rows to rows_dptr (device).  -> rows produced."""
        return self._count('oth_chain_push_dev', dptr, nsamples, rows_dptr, int(capacity))

    def push_async(self, x):
        """work() form: enqueue and return a ticket; the latest row is collected with poll() / wait()."""
        x = _c64(x)
        t = C.c_uint64()
        # direct, not the helper: on the work() path its extra Python call showed (profiles/binding_fold_ab.txt)
        self.ctx.check(self.ctx.lib.oth_chain_push_async(self.h, x.ctypes.data_as(_p), len(x), C.byref(t)), 'oth_chain_push_async')
        return t.value

    def last_push_ops(self):
        """Stream operations (asynchronous copies + kernel launches) the last push enqueued."""
        return self._count('oth_chain_last_push_ops')

    def ticket_rows(self, ticket):
        """Rows the push behind `ticket` produces (known at enqueue time; never waits)."""
        n = C.c_uint64()
        # direct, not the helper: on the work() path its extra Python call showed (profiles/binding_fold_ab.txt)
        self.ctx.check(self.ctx.lib.oth_chain_ticket_rows(self.h, int(ticket), C.byref(n)), 'oth_chain_ticket_rows')
        return n.value

    def poll(self, ticket):
        """-> None while the GPU is still working, else (row or None, rows produced by that push)."""
        row = np.empty(self.nfft, np.float32)
        n, ready = C.c_uint64(), C.c_int()
        # direct, not the helper: on the work() path its extra Python call showed (profiles/binding_fold_ab.txt)
        self.ctx.check(self.ctx.lib.oth_chain_poll(self.h, int(ticket), _fptr(row), C.byref(n), C.byref(ready)), 'oth_chain_poll')
        if not ready.value:
            return None
        return (row if n.value else None), n.value

    def wait(self, ticket):
        row = np.empty(self.nfft, np.float32)
        n = C.c_uint64()
        # direct, not the helper: on the work() path its extra Python call showed (profiles/binding_fold_ab.txt)
        self.ctx.check(self.ctx.lib.oth_chain_wait(self.h, int(ticket), _fptr(row), C.byref(n)), 'oth_chain_wait')
        return (row if n.value else None), n.value

    def peak(self):
        out = np.empty(self.nfft, np.float32)
        self._call('oth_chain_get_peak', _fptr(out))
        return out

    def iir(self):
        out = np.empty(self.nfft, np.float32)
        self._call('oth_chain_get_iir', _fptr(out))
        return out


CHAN_SIZES = (64, 128, 256, 512, 1024, 2048, 4096)      # the channel counts chanpfb.hip is built for
CHAN_TAPS_MAX = 16


def cp_sync_args(hyps):
    """The hypotheses [(Tu, cp), ...] of Context.cp_sync as the library takes them -> (tu int32 [nhyp], cp int32 [nhyp], nhyp,
    the rows' width: the largest Tu + cp, held inside 1 ... 32768 - the library refuses the lengths behind that)."""
    h = np.asarray(hyps, np.int64).reshape(-1, 2)
    tu, cp = np.ascontiguousarray(h[:, 0], np.int32), np.ascontiguousarray(h[:, 1], np.int32)
    row = int(min(max(int((h[:, 0] + h[:, 1]).max()) if len(h) else 1, 1), 32768))
    return tu, cp, len(h), row


def channelizer_args(nchan, decim=None, taps=8, prototype=None):
    """The arguments of Context.channelizer checked and completed without a context -> (nchan, decim, taps, prototype as
    float32 [taps * nchan]); ValueError for what the library would refuse."""
    nchan, taps = int(nchan), int(taps)
    if nchan not in CHAN_SIZES:
        raise ValueError('the channelizer takes a channel count that is a power of two from 64 to 4096, not %d' % nchan)
    decim = nchan // 2 if decim is None else int(decim)
    if decim not in (nchan, nchan // 2, nchan // 4):
        raise ValueError('decim must be nchan, nchan / 2 or nchan / 4 (got %d for %d channels)' % (decim, nchan))
    if not 1 <= taps <= CHAN_TAPS_MAX:
        raise ValueError('taps must lie in 1 ... %d (got %d)' % (CHAN_TAPS_MAX, taps))
    if prototype is None:
        from . import windows
        prototype = windows.pfb_prototype(nchan, taps)
    h = np.ascontiguousarray(np.asarray(prototype, np.float64).ravel(), np.float32)
    if len(h) != taps * nchan:
        raise ValueError('the prototype holds taps * nchan = %d taps, not %d' % (taps * nchan, len(h)))
    if not np.all(np.isfinite(h)):
        raise ValueError('every tap of the prototype must be finite')
    if not np.any(h):
        raise ValueError('the prototype is all zero')
    return nchan, decim, taps, h


class Channelizer(_Handle):
    """Polyphase channelizer with its streaming state on the device (oth_channelizer): one wideband stream in, nchan
    baseband rows out - y_k[m] = sum_n h[n] x[m D + n] exp(-2j pi k (m D + n) / nchan), k in natural (fftfreq) order, the
    phase that of the absolute sample index since creation or reset().  Any split of a stream into pushes gives the same
    bytes as one push."""

    def __init__(self, ctx, nchan, decim=None, taps=8, prototype=None):
        self.nchan, self.decim, self.taps, self.prototype = channelizer_args(nchan, decim, taps, prototype)
        self.ctx = ctx
        h = C.c_void_p()
        ctx._call('oth_channelizer_create', self.nchan, self.decim, self.taps, _fptr(self.prototype), C.byref(h))
        self.h = h

    def close(self):
        if getattr(self, 'h', None) and getattr(self.ctx, 'h', None):
            self.ctx.lib.oth_channelizer_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """the sample count back to 0, the pending tail emptied: the next push gives what a new channelizer gives"""
        self._call('oth_channelizer_reset')

    def frames_for(self, nsamples):
        """frames the NEXT push of nsamples will yield (host arithmetic)"""
        return self._count('oth_channelizer_frames', int(nsamples))

    @property
    def pending(self):
        """samples a later frame still needs, kept on the device: at most taps * nchan - 1"""
        n = C.c_size_t()
        self._call('oth_channelizer_pending', C.byref(n))
        return int(n.value)

    def push(self, x, nsamples=None):
        """Feed samples (a host complex64 array, or a device pointer when nsamples is given); blocking.
        -> complex64 [nchan, frames] of this push, frames possibly 0."""
        src, count, dev = _src(x, nsamples)
        frames = self.frames_for(count)
        out = np.empty((self.nchan, frames), np.complex64)
        n = self._count('oth_channelizer_push', src, count, dev, out.ctypes.data_as(_p) if frames else None, frames)
        assert n == frames
        return out

    def push_dev(self, dptr, nsamples, out_dptr, out_stride):
        """Asynchronous: device-resident samples in, this push's frames to the columns 0 ... frames - 1 of the device
        buffer [nchan][out_stride] complex64 at out_dptr (0 / None where the push yields no frame).  -> frames."""
        return self._count('oth_channelizer_push_dev', dptr, int(nsamples), out_dptr, int(out_stride))

    def last_recipe(self):
        """the launch of the last push that yielded frames (oth__debug_channelizer_recipe); '' before the first"""
        buf = C.create_string_buffer(512)
        self._call('oth__debug_channelizer_recipe', buf, 512)
        return buf.value.decode()

    def channel_freqs(self, fs, fc=0.0):
        """the channels' centres in Hz in the rows' (natural) order: fftfreq(nchan, 1 / fs) + fc"""
        return np.fft.fftfreq(self.nchan, 1.0 / float(fs)) + float(fc)

    def channel_rate(self, fs):
        """the sample rate of every output row: fs / decim"""
        return float(fs) / self.decim


_default_ctx = None


def default_context():
    """Process-wide context on device $OFDM_TOOLS_HIP_DEVICE (default 0, or LOCAL_RANK)."""
    global _default_ctx
    if _default_ctx is None:
        dev = int(os.environ.get('OFDM_TOOLS_HIP_DEVICE', os.environ.get('LOCAL_RANK', '0')))
        _default_ctx = Context(dev)
    return _default_ctx
