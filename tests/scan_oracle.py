"""float64 reference of the scanner's decision stage (moving average, noise floor, channel sums, per-bin mask) and the
row generators of tests/test_scan_decide_gpu.py.  Plain NumPy / math.fsum, independent of the library."""
import math

import numpy as np

from oracle import ref_cpu as R

RTOL_POWER = 1e-5      # channel sums and moving-average outputs (tests/test_hip_parity.py::test_scan_decide_dev_on_device_rows)
RTOL_NOISE = 2e-6      # noise floor (same test, its carrier rows)
MASK_BAND = 8e-6       # a bin within this of the reference level may fall on either side: twice RTOL_NOISE, both ways


def movavg(row, sb):
    """oracle.ref_cpu.movingaverage on the float64 copy of the row."""
    with np.errstate(invalid='ignore', over='ignore'):
        return R.movingaverage(np.asarray(row).astype(np.float64), sb)


def movavg_exact(row, sb):
    """The same outputs with every window summed exactly (math.fsum) before the one division: for rows whose dynamic
    range puts np.convolve's own rounding (M 2^-53 max|tap|) at the size of the noise floor."""
    x = [float(v) for v in np.asarray(row)]
    n, M = len(x), int(sb)
    half = (M - 1) // 2
    out = np.empty(n, np.float64)
    for i in range(n):
        a, b = max(0, i + half - M + 1), min(n, i + half + 1)      # taps n = i + half - j, j in [0, M)
        out[i] = abs(math.fsum(x[a:b]) / float(sb))
    return out


def noise_of(ma):
    """Row minimum as numpy takes it (a NaN stays), rounded to float32."""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.float32(np.min(ma))


def channel_sums(ma, lo, hi):
    """sum(ma[lo:hi]) with Python slice semantics, in float64."""
    with np.errstate(invalid='ignore', over='ignore'):
        return np.array([np.sum(ma[int(a):int(b)], dtype=np.float64) for a, b in zip(lo, hi)], np.float64)


def mask_of(row, thr, noise):
    """row > float32(thr) * float32(noise) -> (mask uint8, the float32 level)."""
    with np.errstate(invalid='ignore', over='ignore'):
        level = np.float32(thr) * np.float32(noise)
        return (np.asarray(row, np.float32) > level).astype(np.uint8), level


class Ref(object):
    """Reference results of rows [nrows][nfft]: ma float64, noise float32[nrows], power float64[nrows][nch],
    mask uint8 and the float32 level it was taken at."""

    def __init__(self, rows, sb, thr, lo=(), hi=(), exact=False):
        rows = np.atleast_2d(np.asarray(rows, np.float32))
        f = movavg_exact if exact else movavg
        self.rows = rows
        self.ma = np.stack([f(r, sb) for r in rows])
        self.noise = np.array([noise_of(m) for m in self.ma], np.float32)
        self.power = (np.stack([channel_sums(m, lo, hi) for m in self.ma]) if len(lo)
                      else np.zeros((len(rows), 0), np.float64))
        ml = [mask_of(r, thr, n) for r, n in zip(rows, self.noise)]
        self.mask = np.stack([m for m, _ in ml])
        self.level = np.array([v for _, v in ml], np.float32)

    def head(self, n):
        """The first n rows of the same reference."""
        r = object.__new__(Ref)
        r.rows, r.ma, r.noise, r.power, r.mask, r.level = (self.rows[:n], self.ma[:n], self.noise[:n], self.power[:n],
                                                            self.mask[:n], self.level[:n])
        return r


def gamma_rows(nrows, nfft, seed):
    """1e-9 * gamma(4, 0.25) float32 rows with about 2 % of the bins raised by 20 dB."""
    rng = np.random.default_rng(seed)
    rows = 1e-9 * rng.gamma(4.0, 0.25, (nrows, nfft))
    rows[rng.random((nrows, nfft)) < 0.02] *= 100.0
    return rows.astype(np.float32)


def even_slices(nfft, nch):
    """nch slices that tile [0, nfft) (the last one ends at nfft), like the scanner's channels."""
    edges = np.linspace(0, nfft, nch + 1).astype(np.int64)
    return edges[:-1].astype(np.int32), edges[1:].astype(np.int32)


def relerr(got, ref):
    """Largest |got - ref| / |ref| over the finite, non-zero reference values (0 when there is none)."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    ok = np.isfinite(ref) & (ref != 0)
    if not ok.any():
        return 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        return float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok])))
