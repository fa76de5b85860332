"""What the seeded random-shape generators (stat_fuzz_cases.py, core_fuzz_cases.py) share - a plain module, no fixtures, no
GPU: the NaN-fenced input buffer, the NaN tail of a lane, the guarded output row blocks and the single-precision transform
that stands in for np.fft.fft in an oracle."""
import contextlib

import numpy as np

from call_order_cases import GUARD, SENTINEL

NAN64 = np.complex64(complex(np.nan, np.nan))
BEHIND = 64                # samples behind the last stream


# ---- the input ------------------------------------------------------------------------------------------------------------------

def nan_tail(lane, owned):
    """one lane as the layout holds it: everything behind its first `owned` samples reads NaN"""
    out = np.array(lane, np.complex64)
    out[..., owned:] = NAN64
    return out


def nan_buffer(data, lead, stride, nsamples, owned, tails=None):
    """-> complex64 [lead + (L - 1) stride + nsamples + BEHIND], NaN everywhere but the first `owned` samples of each of the
    L lanes of `data` ([L][>= owned]), lane i at lead + i stride.  tails: [L][nsamples - owned] finite samples that fill the
    tail inside nsamples (a route that reads it), else the tail is NaN too."""
    L = len(data)
    buf = np.full(lead + (L - 1) * stride + nsamples + BEHIND, NAN64, np.complex64)
    for i in range(L):
        buf[lead + i * stride:lead + i * stride + owned] = data[i][:owned]
        if tails is not None:
            buf[lead + i * stride + owned:lead + i * stride + nsamples] = tails[i]
    return buf


# ---- the output -----------------------------------------------------------------------------------------------------------------

def row_block(units, width):
    """the words of one output row block: GUARD, `units` rows of `width` floats, a spare row, GUARD - all SENTINEL.  The
    call's pointer is GUARD words in."""
    return np.full(2 * GUARD + (units + 1) * width, SENTINEL, np.uint32)


def rows_of_block(words, units, width, name, text):
    """The block read back: asserts guards and spare row still the sentinel and no sentinel left in a written row
    -> float32 [units][width]"""
    assert words.shape == (2 * GUARD + (units + 1) * width,)
    assert np.all(words[:GUARD] == SENTINEL) and np.all(words[GUARD + units * width:] == SENTINEL), \
        'row %s: a guard or the spare row was written [%s]' % (name, text)
    body = words[GUARD:GUARD + units * width]
    assert not np.any(body == SENTINEL), 'row %s: %d words left unwritten [%s]' % (name, int(np.sum(body == SENTINEL)), text)
    return body.view(np.float32).reshape(units, width)


# ---- float32 transform in the oracles' place ------------------------------------------------------------------------------------

def _fft32(a, n=None, axis=-1):
    import scipy.fft
    out = scipy.fft.fft(np.asarray(a).astype(np.complex64), n, axis)
    assert out.dtype == np.complex64
    return out.astype(np.complex128)


@contextlib.contextmanager
def float32_transform():
    """np.fft.fft is pocketfft's single-precision transform inside: the input cast to complex64, the result back to
    complex128; everything else of an oracle stays float64"""
    old = np.fft.fft
    np.fft.fft = _fft32
    try:
        yield
    finally:
        np.fft.fft = old
