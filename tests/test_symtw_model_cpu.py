"""Float32 NumPy model of welch4096ws's complementary-window build: the three radix-16 passes on signed digits around the
time origin n' = n - 136, with the two inter-pass twiddle layers as three-shear rotations (twiddle16.hip.h, rot3).

    n' = 256 a + 16 (b - 8) + (c - 8),   k = kappa + 16 lambda + 256 mu (mod 4096),  kappa, lambda in [-8, 8), mu in [0, 16)
    pass 1 (over a) -> digit k0, twiddle e^(-2 pi i kappa tau / 4096), tau = 16 (b - 8) + (c - 8) = t - 136
    pass 2 (over b) -> digit k1, twiddle e^(-2 pi i lambda (c - 8) / 256)
    pass 3 (over c) -> register mu of consumer thread (k0, k1)

The butterflies are plain 16-point DFTs on the unshifted digits b, c, which leaves (-1)^lambda on every input of a pass-3
transform and (-1)^mu on its output; with the unit phase of the shifted origin none of it survives |X|^2.  The tables are
built the way the library builds them (abi_ctx.hip symtw_table, abi_welch.hip window_spectrum_table_sym): in double,
rounded once to float32.  The library has no query that returns a plan's tables, so they are restated here.
"""
import numpy as np
import pytest

SHIFT, ORIGIN = 136, 1100
F = np.float32


def sym16(k):
    return k if k < 8 else k - 16


def symtw_table():
    e = np.arange(-ORIGIN, ORIGIN + 1, dtype=np.float64)
    a = 2.0 * np.pi * e / 4096.0
    return np.tan(0.5 * a).astype(F), np.sin(a).astype(F)


TAN, SIN = symtw_table()


def rot3(x, y, e, conj):
    """(x + i y) e^(-i theta) (conj: e^(+i theta)), theta = 2 pi e / 4096, as three float32 fused multiply-adds; the
    products are formed in float64 - exact for float32 factors - and the sum rounded once"""
    t, s = TAN[ORIGIN + e], SIN[ORIGIN + e]
    if conj:
        t, s = -t, -s
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    x1 = fma(t, y, x)
    y1 = fma(-s, x1, y)
    return fma(t, y1, x1), y1


def dft16(z, axis):
    """16-point DFT of complex64 data along `axis`, rounded to complex64"""
    k = np.arange(16)
    m = np.exp(-2j * np.pi * np.outer(k, k) / 16.0)
    return np.moveaxis(np.tensordot(m, z.astype(np.complex128), axes=([1], [axis])), 0, axis).astype(np.complex64)


def twiddle_layer(z, step):
    """z[digit][...] times e^(-2 pi i sym16(digit) step / 4096) with the eight stored pairs of |digit|; step: int array
    broadcast against z[digit]"""
    out = np.empty_like(z)
    out[0] = z[0]
    for k in range(1, 16):
        d = sym16(k)
        x, y = rot3(z[k].real.astype(F), z[k].imag.astype(F), abs(d) * step, d < 0)
        out[k] = x + 1j * y
    return out


def transform(x):
    """-> Y[k0][k1][mu] complex64 of 4096 complex64 samples"""
    v = x.astype(np.complex64).reshape(16, 16, 16)                # [a][b][c]
    y = dft16(v, 0)                                               # [k0][b][c]
    b, c = np.meshgrid(np.arange(16), np.arange(16), indexing='ij')
    y = twiddle_layer(y, 16 * (b - 8) + (c - 8))
    y = dft16(y, 1)                                               # [k0][k1][c]
    y = np.moveaxis(twiddle_layer(np.moveaxis(y, 1, 0), 16 * (np.arange(16) - 8)[None, :]), 0, 1)
    return dft16(y, 2)                                            # [k0][k1][mu]


def bin_of(k0, k1, mu):
    return (sym16(k0) + 16 * sym16(k1) + 256 * mu) % 4096


def store_position(k0, k1, mu):
    """the kernel's final store: where register mu of thread (k0, k1) goes in a finalize layout 1 row"""
    g = k0 >> 3
    down = (k1 >> 3) + (g if k1 == 0 else 0)
    return ((256 * mu - 256 * down) & 4095) + 16 * k0 + ((k1 - g) & 15)


def fd_sym(w):
    """window_spectrum_table_sym: per thread t = 16 k0 + k1 the re-phased, signed FFT(w) at its mu = 0 bin"""
    fw = np.fft.fft(np.asarray(w, np.float32).astype(np.float64))
    out = np.empty(256, np.complex64)
    for t in range(256):
        lam = sym16(t & 15)
        k = sym16(t >> 4) + 16 * lam
        out[t] = (-1.0) ** (lam & 1) * np.exp(2j * np.pi * ((SHIFT * k) % 4096) / 4096.0) * fw[k % 4096]
    return out


def test_tangents_stay_small_and_exponents_inside_the_table():
    exps = [m * (t - SHIFT) for m in range(1, 9) for t in range(256)] + [16 * m * (c - 8) for m in range(1, 9) for c in range(16)]
    assert max(abs(e) for e in exps) <= 8 * SHIFT < ORIGIN
    assert float(np.max(np.abs(TAN))) < 1.2 and float(np.max(np.abs(SIN))) <= 1.0
    assert max(abs(float(TAN[ORIGIN + e])) for e in exps) < 1.2


def test_register_to_bin_map_is_a_permutation_and_mu0_is_the_window_band():
    bins = [bin_of(k0, k1, mu) for k0 in range(16) for k1 in range(16) for mu in range(16)]
    assert sorted(bins) == list(range(4096))
    mu0 = sorted((sym16(k0) + 16 * sym16(k1)) for k0 in range(16) for k1 in range(16))
    assert mu0 == list(range(-SHIFT, 120))
    # the store puts bin k0' + 16 k1' + 256 k2' at 256 k2' + 16 k0' + k1' (finalize layout 1), each position once
    seen = set()
    for k0 in range(16):
        for k1 in range(16):
            for mu in range(16):
                k = bin_of(k0, k1, mu)
                pos = store_position(k0, k1, mu)
                assert pos == 256 * (k >> 8) + 16 * (k & 15) + ((k >> 4) & 15), (k0, k1, mu, k, pos)
                seen.add(pos)
    assert len(seen) == 4096


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_power_spectrum_agrees_with_numpy(seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex64)
    x += (3.0 * np.exp(2j * np.pi * 0.1234 * np.arange(4096))).astype(np.complex64)
    Y = transform(x)
    ref = np.abs(np.fft.fft(x.astype(np.complex128))) ** 2
    got = np.empty(4096)
    for k0 in range(16):
        for k1 in range(16):
            for mu in range(16):
                got[bin_of(k0, k1, mu)] = abs(complex(Y[k0, k1, mu])) ** 2
    err = float(np.max(np.abs(got - ref)) / np.max(ref))
    print('max |X|^2 error / peak: %.2e' % err)
    assert err < 1e-5


@pytest.mark.parametrize('name', ['hann', 'flattop'])
def test_rephased_table_cancels_a_constant_input(name):
    """x = m everywhere: Y - m fd_sym is (numerically) zero at bins -4..4, the whole reach of both windows.  What is left
    is the rounding of a float32 transform whose largest output is `peak`: 4e-6 of it is 32 float32 ulp (2^-23), room for
    the three passes' roundings (each a few ulp of the peak at most) and none for a wrong phase or sign, which leaves the
    whole of |m FFT(w)[k]| - from a hundredth of the peak (flattop, k = +-4) to the peak itself - behind"""
    from ofdm_tools import windows
    w = np.asarray(windows.get_window(name, 4096), np.float32)
    m = 3.0 - 2.0j
    Y = transform((m * w).astype(np.complex64))
    fd = fd_sym(w)
    peak = abs(m) * float(np.sum(w))
    for k in range(-4, 5):
        k0, k1 = k % 16, ((k - sym16(k % 16)) // 16) % 16
        assert bin_of(k0, k1, 0) == k % 4096
        left = abs(complex(Y[k0, k1, 0]) - m * complex(fd[16 * k0 + k1]))
        assert left < 4e-6 * peak, (name, k, left / peak)
    # and nothing of the window lies outside the registers mu = 0
    fw = np.abs(np.fft.fft(w.astype(np.float64))) ** 2
    assert np.all(fw[120:4096 - SHIFT] <= 1e-10 * float(np.sum(w.astype(np.float64) ** 2)))
