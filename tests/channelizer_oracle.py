"""float64 oracle of the polyphase channelizer (oth_channelizer, csrc/chanpfb.hip) by the definition, with no fold: per
channel k the input is mixed by exp(-2j pi k t / M) with t the absolute sample index, filtered with the prototype h of L taps
and every D-th output is kept,
    y_k[m] = sum_{n < L} h[n] x[m D + n] exp(-2j pi k (m D + n) / M),
k in natural order.  The phase is formed from (k t) mod M in integers, so it is exact at any t.  A second function gives the
computed form - fold, circular shift, transform - in float64: tests/test_channelizer_cpu.py holds it to the definition, and
the GPU suite uses it where all M channels of a large bank are wanted (the definition costs L products per output)."""
import numpy as np


def frames(pending, nsamples, L, D):
    """frames the next push of nsamples yields with `pending` samples kept"""
    total = pending + nsamples
    return (total - L) // D + 1 if total >= L else 0


def frame_view(z, L, D, count):
    """[count, L] view of z: row m holds z[m D : m D + L]"""
    z = np.ascontiguousarray(z)
    return np.lib.stride_tricks.as_strided(z, (count, L), (D * z.strides[0], z.strides[0]), writeable=False)


def channelize(x, nchan, decim, h, channels=None, t0=0):
    """By the definition -> complex128 [len(channels), frames]; channels: the rows wanted (all by default), t0 the absolute
    index of x[0] (a multiple of decim: a frame starts there)."""
    x = np.asarray(x, np.complex128)
    h = np.asarray(h, np.float64)
    M, D, L = int(nchan), int(decim), len(h)
    count = frames(0, len(x), L, D)
    channels = range(M) if channels is None else channels
    out = np.zeros((len(channels), count), np.complex128)
    if not count:
        return out
    t = np.arange(len(x), dtype=np.int64) + int(t0)
    for i, k in enumerate(channels):
        z = x * np.exp(-2j * np.pi * ((int(k) * t) % M) / M)      # mixed to DC
        out[i] = frame_view(z, L, D, count) @ h                     # filtered, every D-th output
    return out


def bound(x, decim, h, frame_list=None):
    """sum_n |h[n]| |x[m D + n]| per frame (all of them, or those of frame_list): the size of the worst-case output, of
    which every rounding is a fraction"""
    a = np.abs(np.asarray(x, np.complex128))
    h = np.abs(np.asarray(h, np.float64))
    L, D = len(h), int(decim)
    if frame_list is not None:
        return np.array([a[m * D:m * D + L] @ h for m in frame_list])
    return frame_view(a, L, D, frames(0, len(a), L, D)) @ h


def channelize_fold(x, nchan, decim, h, frame_list=None, frame0=0):
    """The computed form in float64 -> complex128 [nchan, len(frame_list)]: u_m[r] = sum_p h[r + p M] x[m D + r + p M],
    v_m[(r + (frame0 + m) D) mod M] = u_m[r], y[:, m] = FFT_M(v_m); frame_list: the frames wanted (all by default)."""
    x = np.asarray(x, np.complex128)
    h = np.asarray(h, np.float64)
    M, D, L = int(nchan), int(decim), len(h)
    if frame_list is None:
        frame_list = range(frames(0, len(x), L, D))
    out = np.zeros((M, len(frame_list)), np.complex128)
    for i, m in enumerate(frame_list):
        u = (x[m * D:m * D + L] * h).reshape(L // M, M).sum(axis=0)
        out[:, i] = np.fft.fft(np.roll(u, ((frame0 + m) * D) % M))
    return out
