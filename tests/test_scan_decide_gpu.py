"""The scanner's decision stage (oth_scan_decide_dev / oth_scan_decide_dev_out: movavg_run_kernel + scan_post_kernel, or
movavg_kernel + channel_sum_kernel + bin_threshold_ma_kernel behind the other door of launch_scan_decide) and the
host-row small ops (oth_channel_power, oth_bin_threshold, oth_rows_group_mean) against a plain float64 reference
(tests/scan_oracle.py) over row lengths, window lengths, alignments, slice layouts and hard rows.

Tolerances are the ones of test_hip_parity.py::test_scan_decide_dev_on_device_rows (noise floor 2e-6, channel power
1e-5); every case prints the largest error it saw ('scan-err ...', pytest -s) - DESIGN.md section 2 carries the table.
The mask is compared with the REFERENCE's mask; a bin within 8e-6 of the reference level may fall on either side and is
left out, at most max(1, nfft // 1000) bins per row.  Device outputs are filled with a sentinel first, so an output a
kernel never wrote shows."""
import numpy as np
import pytest

import scan_oracle as S
from oracle import ref_cpu as R
from test_hip_parity import ctx, hip  # noqa: F401 - fixtures

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_HIP = -1, -2
SENT = 0xA5                       # byte the device outputs are filled with before a call
SENT32 = 0xA5A5A5A5


# ---- plumbing -----------------------------------------------------------------------------------------------------

class DevRows(object):
    """Rows uploaded `off` bytes into a device allocation."""

    def __init__(self, ctx, rows, off=0):
        self.ctx = ctx
        self.rows = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
        self.nrows, self.nfft = self.rows.shape
        self.base = ctx.alloc(self.rows.nbytes + 16)
        self.ptr = self.base + off
        ctx.h2d(self.ptr, self.rows)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.sync()
        self.ctx.free(self.base)


class Out(object):
    """Sentinel-filled device outputs of one oth_scan_decide_dev_out call."""

    def __init__(self, ctx, nrows, nfft, nch, mask_off=0, want_mask=True):
        self.ctx, self.shape, self.nch, self.want_mask = ctx, (nrows, nfft), nch, want_mask
        self.sizes = (nrows * nfft + 4, 4 * nrows, 4 * nrows * max(nch, 1))
        self.ptrs = [ctx.alloc(n) for n in self.sizes]
        for p, n in zip(self.ptrs, self.sizes):
            ctx.h2d(p, np.full(n, SENT, np.uint8))
        self.mask_ptr = self.ptrs[0] + mask_off

    def launch(self, d, sb, thr, lo, hi):
        self.ctx.scan_decide_dev_out(d.ptr, d.nrows, d.nfft, sb, thr, lo, hi, self.ptrs[1], self.ptrs[2],
                                     self.mask_ptr if self.want_mask else 0)

    def read(self):
        nrows, nfft = self.shape
        raw = self.ctx.d2h(self.ptrs[0], (self.sizes[0],), np.uint8)
        off = self.mask_ptr - self.ptrs[0]
        if self.want_mask:
            mask = raw[off:off + nrows * nfft].reshape(nrows, nfft).copy()
            raw[off:off + nrows * nfft] = SENT
        assert np.all(raw == SENT), 'bytes outside the mask were written' if self.want_mask else 'a mask was written'
        noise = self.ctx.d2h(self.ptrs[1], (nrows,), np.float32)
        power = self.ctx.d2h(self.ptrs[2], (nrows, max(self.nch, 1)), np.float32)
        if self.nch == 0:
            assert np.all(power.view(np.uint32) == SENT32), 'power written with nch = 0'
            power = power[:, :0]
        return (mask if self.want_mask else None), noise, power

    def free(self):
        self.ctx.sync()
        for p in self.ptrs:
            self.ctx.free(p)


def dev_out(ctx, d, sb, thr, lo=(), hi=(), mask_off=0, want_mask=True):
    """oth_scan_decide_dev_out on DevRows d -> (mask or None, noise, power), read back after ctx.sync()."""
    o = Out(ctx, d.nrows, d.nfft, len(lo), mask_off, want_mask)
    try:
        o.launch(d, sb, thr, lo, hi)
        ctx.sync()
        return o.read()
    finally:
        o.free()


def check(got, ref, lo=(), hi=(), floor=0.0, thr=0.0):
    """(mask or None, noise, power or None) of the library against a scan_oracle.Ref -> (largest relative error of the
    noise floor, of the channel powers).  `floor`: absolute error allowed per moving-average output on top of the
    relative tolerance (0 except on mixed-sign rows, see there)."""
    mask, noise, power = got
    nrows, nfft = ref.rows.shape
    assert noise.shape == (nrows,)
    assert not np.any(noise.view(np.uint32) == SENT32), 'noise floor never written'
    for i in range(nrows):
        r, g = float(ref.noise[i]), float(noise[i])
        if np.isnan(r):
            assert np.isnan(g), (i, g)
        elif r == 0.0 or np.isinf(r):
            assert g == r, (i, g, r)
        else:
            assert abs(g - r) <= S.RTOL_NOISE * abs(r) + floor, (i, g, r, abs(g - r) / abs(r))
    if power is not None:
        assert power.shape == ref.power.shape
        assert not np.any(power.view(np.uint32) == SENT32), 'channel power never written'
        with np.errstate(over='ignore', invalid='ignore'):
            ref32 = ref.power.astype(np.float32)
            wild = ~np.isfinite(ref32)
            assert np.array_equal(power[wild], ref32[wild], equal_nan=True), (power[wild], ref32[wild])
            width = np.maximum(1, np.asarray(hi, np.int64) - np.asarray(lo, np.int64)) if len(lo) else 1
            bad = ~wild & ~(np.abs(power - ref.power) <= S.RTOL_POWER * np.abs(ref.power) + floor * width)
        assert not bad.any(), (np.argwhere(bad)[:5], power[bad][:5], ref.power[bad][:5])
    if mask is not None:
        assert mask.shape == (nrows, nfft) and mask.max() <= 1, 'mask bytes never written, or not 0 / 1'
        for i in range(nrows):
            lvl = float(ref.level[i])
            if np.isnan(lvl):
                assert not mask[i].any(), i                  # NaN noise floor: nothing is above it
                continue
            if np.isinf(lvl) or lvl == 0.0:
                near = np.zeros(nfft, bool)                  # row > inf and row > 0 have no rounding to allow for
            else:
                near = np.abs(ref.rows[i].astype(np.float64) - lvl) <= S.MASK_BAND * abs(lvl) + 2.0 * thr * floor
            assert near.sum() <= max(1, nfft // 1000), (i, int(near.sum()))
            diff = (mask[i] != ref.mask[i]) & ~near
            assert not diff.any(), (i, np.flatnonzero(diff)[:8], lvl)
    return (S.relerr(noise, ref.noise), S.relerr(power, ref.power) if power is not None else 0.0)


def bit_equal(a, b):
    """Two (mask, noise, power) results are the same bits."""
    (ma, na, pa), (mb, nb, pb) = a, b
    assert (ma is None) == (mb is None)
    if ma is not None:
        assert np.array_equal(ma, mb)
    assert np.array_equal(na.view(np.uint32), nb.view(np.uint32)), (na, nb)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))


def masks_agree(a, b, ref):
    """Two masks of the same rows agree outside the bins that lie on the reference level."""
    for i in range(len(ref.rows)):
        lvl = float(ref.level[i])
        near = np.abs(ref.rows[i].astype(np.float64) - lvl) <= S.MASK_BAND * abs(lvl)
        assert np.array_equal(a[i][~near], b[i][~near]), i


def both_entries(ctx, rows, sb, thr, lo=(), hi=()):
    """Host-result and device-result entry point on the same rows: the same kernels on the same inputs, so the same
    bits.  -> the host form's (mask, noise, power)."""
    with DevRows(ctx, rows) as d:
        host = ctx.scan_decide_dev(d.ptr, d.nrows, d.nfft, sb, thr, lo, hi)
        out = dev_out(ctx, d, sb, thr, lo, hi)
    bit_equal(host, out)
    return host


def refused(ctx, call, what=None):
    """`call` raises HipError(OTH_ERR_INVALID) with a message."""
    from ofdm_tools._hip import HipError
    with pytest.raises(HipError) as e:
        call()
    assert e.value.code == ERR_INVALID, e.value
    text = str(e.value).split('):', 1)[1].strip()
    assert text and (what is None or what in text), str(e.value)


# ---- 2. shapes ----------------------------------------------------------------------------------------------------

NFFTS = [4, 8, 12, 64, 1000, 1004, 4096, 4100, 4104, 16384, 20000, 65536, 1021, 4099, 10007, 4098]
SBS = [1.0, 1.5, 2.0, 7.9, 8.0, 9.0, 163.84, 1023.99, 1024.0, 1024.5, 1025.0, 2000.0]


def door(nfft, sb):
    """The implementation launch_scan_decide picks for aligned pointers."""
    return 'tiled' if nfft % 4 == 0 and int(sb) <= 1024 else 'direct'


def shape_cases():
    """Every window length at 4100 and 65536 bins; every row length with M = 1, an even M, an odd M, M = 163 and
    M = 1024 on the tiled door where they fit, and the largest M of the list that fits."""
    out = []
    for nfft in NFFTS:
        fit = [sb for sb in SBS if int(sb) <= nfft]
        pick = fit if nfft in (4100, 65536) else sorted(set([1.0, 2.0, fit[-1]] +
                                                            [sb for sb in (9.0, 163.84, 1024.5) if sb in fit]))
        out += [(nfft, sb) for sb in pick]
    return out


SHAPES = shape_cases()
SHAPE_IDS = ['n%d-sb%s-%s' % (n, sb, door(n, sb)) for n, sb in SHAPES]
THRS = (1.5, 3.0, 10.0)


def thr_of(nfft, sb):
    return THRS[(SHAPES.index((nfft, sb))) % 3]


@pytest.mark.parametrize('nfft,sb', SHAPES, ids=SHAPE_IDS)
def test_decide_shapes(ctx, nfft, sb):
    """oth_scan_decide_dev and _dev_out on 1, 3 and 64 rows: partial tiles, cut runs, rows shorter than a tile, 16
    tiles, both doors, M from 1 to 2000 (64 rows where the float64 reference of 64 rows is cheap)."""
    thr = thr_of(nfft, sb)
    nmax = 64 if nfft * int(sb) <= 2e6 else 3
    rows = S.gamma_rows(nmax, nfft, 1000 * nfft + int(100 * sb))
    lo, hi = S.even_slices(nfft, min(nfft, 7))
    ref = S.Ref(rows, sb, thr, lo, hi)
    assert any(0 < int(m.sum()) < nfft for m in ref.mask), 'no row of this case has bins on both sides of the level'
    errs = []
    for nrows in (1, 3, 64):
        if nrows <= nmax:
            errs.append(check(both_entries(ctx, rows[:nrows], sb, thr, lo, hi), ref.head(nrows), lo, hi))
    print('scan-err decide n%d sb%s %s noise %.3g power %.3g' % (nfft, sb, door(nfft, sb), max(e[0] for e in errs),
                                                                max(e[1] for e in errs)))


@pytest.mark.parametrize('nfft', [4100, 16384])
def test_alignment_doors_agree(ctx, nfft):
    """Rows that start 4 bytes into an allocation and a mask pointer 1 byte in take the direct kernels; the same rows at
    aligned addresses the tiled ones.  Both are right, and their masks agree."""
    sb, thr = 163.84, 3.0
    rows = S.gamma_rows(3, nfft, 77 + nfft)
    lo, hi = S.even_slices(nfft, 7)
    ref = S.Ref(rows, sb, thr, lo, hi)
    with DevRows(ctx, rows) as d:
        aligned = dev_out(ctx, d, sb, thr, lo, hi)
        odd_mask = dev_out(ctx, d, sb, thr, lo, hi, mask_off=1)
    with DevRows(ctx, rows, off=4) as d:
        odd_rows = dev_out(ctx, d, sb, thr, lo, hi)
        odd_rows_host = ctx.scan_decide_dev(d.ptr, 3, nfft, sb, thr, lo, hi)
    bit_equal(odd_rows, odd_rows_host)
    for name, got in (('aligned', aligned), ('mask+1', odd_mask), ('rows+4', odd_rows)):
        e = check(got, ref, lo, hi)
        print('scan-err align n%d %s noise %.3g power %.3g' % (nfft, name, e[0], e[1]))
    masks_agree(aligned[0], odd_mask[0], ref)
    masks_agree(aligned[0], odd_rows[0], ref)
    assert np.allclose(aligned[1], odd_rows[1], rtol=2 * S.RTOL_NOISE, atol=0)
    assert np.allclose(aligned[2], odd_mask[2], rtol=2 * S.RTOL_POWER, atol=0)


@pytest.mark.parametrize('nfft', [4100, 4099])
def test_without_mask_and_without_channels(ctx, nfft):
    sb, thr = 9.0, 3.0
    rows = S.gamma_rows(3, nfft, 5 + nfft)
    lo, hi = S.even_slices(nfft, 5)
    ref = S.Ref(rows, sb, thr, lo, hi)
    with DevRows(ctx, rows) as d:
        full = ctx.scan_decide_dev(d.ptr, 3, nfft, sb, thr, lo, hi)
        host = ctx.scan_decide_dev(d.ptr, 3, nfft, sb, thr, lo, hi, want_mask=False)
        out = dev_out(ctx, d, sb, thr, lo, hi, want_mask=False)
        assert host[0] is None and out[0] is None
        bit_equal(host, out)
        bit_equal(host, (None,) + full[1:])
        check(host, ref, lo, hi)
        host0 = ctx.scan_decide_dev(d.ptr, 3, nfft, sb, thr)                  # nch = 0: null bounds and power
        out0 = dev_out(ctx, d, sb, thr)
        assert host0[2].shape == (3, 0)
        bit_equal(host0, out0)
        bit_equal((host0[0], host0[1], full[2]), full)
        none = dev_out(ctx, d, sb, thr, want_mask=False)                         # neither: the noise floor alone
        assert np.array_equal(none[1].view(np.uint32), full[1].view(np.uint32))


# ---- 3. slices and the bounds cache ---------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft', [4100, 20000])
def test_channel_counts(ctx, nfft):
    """nch around the four-slices-per-workgroup grouping of scan_post_kernel, up to 1000."""
    sb, thr = 163.84, 3.0
    rows = S.gamma_rows(3, nfft, 31 + nfft)
    for nch in (1, 2, 3, 4, 5, 7, 64, 127, 1000):
        lo, hi = S.even_slices(nfft, nch)
        check(both_entries(ctx, rows, sb, thr, lo, hi), S.Ref(rows, sb, thr, lo, hi), lo, hi)


@pytest.mark.parametrize('nfft', [4100, 20000, 4099])
def test_slice_layouts(ctx, nfft):
    """Empty and inverted slices, the whole row, one-bin slices at both ends, slices across tile edges, overlapping and
    unsorted ones - Python slice semantics."""
    sb, thr = 163.84, 3.0
    top = min(nfft, 8400)
    sl = [(5, 5), (900, 300), (0, nfft), (0, 1), (nfft - 1, nfft), (4000, min(nfft, 4100)), (4095, 4097), (top - 400, top),
          (100, 900), (500, 1500), (3000, 3100), (10, 20), (nfft, nfft), (0, 0)]
    lo, hi = np.array([a for a, _ in sl], np.int32), np.array([b for _, b in sl], np.int32)
    rows = S.gamma_rows(3, nfft, 41 + nfft)
    ref = S.Ref(rows, sb, thr, lo, hi)
    assert np.all(ref.power[:, [0, 1, 12, 13]] == 0)
    got = both_entries(ctx, rows, sb, thr, lo, hi)
    check(got, ref, lo, hi)
    assert np.all(got[2][:, [0, 1, 12, 13]] == 0)


def test_refusals_leave_the_context_usable(ctx):
    nfft, thr = 4100, 3.0
    rows = S.gamma_rows(2, nfft, 51)
    lo, hi = S.even_slices(nfft, 5)
    ref = S.Ref(rows, 9.0, thr, lo, hi)
    with DevRows(ctx, rows) as d:
        o = Out(ctx, 2, nfft, 5)
        try:
            bad = [(9.0, [-1, 5], [3, 9], 'slice'), (9.0, [0, 5], [3, nfft + 1], 'slice'), (0.5, [0], [1], 'srch_bins'),
                   (float('nan'), [0], [1], 'srch_bins'), (0.5, (), (), 'srch_bins'), (float('nan'), (), (), 'srch_bins')]
            for sb, blo, bhi, what in bad:
                refused(ctx, lambda: ctx.scan_decide_dev(d.ptr, 2, nfft, sb, thr, blo, bhi), what)
                refused(ctx, lambda: ctx.scan_decide_dev_out(d.ptr, 2, nfft, sb, thr, blo, bhi, o.ptrs[1], o.ptrs[2],
                                                             o.ptrs[0]), what)
                check(ctx.scan_decide_dev(d.ptr, 2, nfft, 9.0, thr, lo, hi), ref, lo, hi)
            ctx.sync()
            assert o.read()[1].view(np.uint32).tolist() == [SENT32] * 2      # a refused call wrote nothing
        finally:
            o.free()
    refused(ctx, lambda: ctx.bin_threshold(rows, 0.5, thr), 'srch_bins')
    refused(ctx, lambda: ctx.bin_threshold(rows, float('nan'), thr), 'srch_bins')
    refused(ctx, lambda: ctx.channel_power(rows[0], 0.5, [0], [1]), 'srch_bins')
    refused(ctx, lambda: ctx.channel_power(rows[0], 9.0, [-1], [1]), 'slice')
    refused(ctx, lambda: ctx.channel_power(rows[0], 9.0, [0], [nfft + 1]), 'slice')
    m, n = ctx.bin_threshold(rows, 9.0, thr)
    check((m, n, None), ref)


def fresh(hip, d, sb, thr, lo, hi):
    """What a context that has never seen other bounds computes."""
    c = hip.Context(0)
    try:
        return c.scan_decide_dev(d.ptr, d.nrows, d.nfft, sb, thr, lo, hi)
    finally:
        c.close()


def test_bounds_cache(ctx, hip):
    """channel_bounds_dev keeps the last slice bounds on the device: equal counts with other values (same lo and other
    hi, and the reverse), growth past the cached capacity and back, the same values permuted - through both entry
    points, each result the bits a fresh context gives."""
    nfft, sb, thr = 4100, 163.84, 3.0
    rows = S.gamma_rows(3, nfft, 61)
    lo_a, hi_a = S.even_slices(nfft, 5)
    A = (lo_a, hi_a)
    B = (lo_a, np.minimum(hi_a + 37, nfft).astype(np.int32))       # lo as A, other hi
    Cc = (np.maximum(lo_a - 11, 0).astype(np.int32), hi_a)         # hi as A, other lo
    big = S.even_slices(nfft, 200)
    small = S.even_slices(nfft, 3)
    perm = (lo_a[::-1].copy(), hi_a[::-1].copy())
    with DevRows(ctx, rows) as d:
        want = {id(b): fresh(hip, d, sb, thr, *b) for b in (A, B, Cc, big, small, perm)}
        assert not np.array_equal(want[id(A)][2], want[id(B)][2]) and not np.array_equal(want[id(A)][2], want[id(Cc)][2])
        check(want[id(A)], S.Ref(rows, sb, thr, *A), *A)
        for b in (A, B, A, A, Cc, A, big, small, A, perm, A, perm, big, B):
            bit_equal(dev_out(ctx, d, sb, thr, *b), want[id(b)])
            bit_equal(ctx.scan_decide_dev(d.ptr, 3, nfft, sb, thr, *b), want[id(b)])


def test_two_bounds_back_to_back_behind_a_busy_stream(ctx, hip):
    """Two _dev_out calls with different bounds enqueued without a sync while the stream is still busy with earlier
    work: the second upload must not reach the kernels of the first."""
    from test_chain_async_gpu import Hog
    nfft, sb, thr = 20000, 163.84, 3.0
    rows = S.gamma_rows(3, nfft, 71)
    A = S.even_slices(nfft, 7)
    B = (A[0], np.minimum(A[1] + 501, nfft).astype(np.int32))
    hog = Hog(ctx, hip)
    try:
        with DevRows(ctx, rows) as d:
            want_a, want_b = fresh(hip, d, sb, thr, *A), fresh(hip, d, sb, thr, *B)
            assert not np.array_equal(want_a[2], want_b[2])
            dev_out(ctx, d, sb, thr, *B)                      # the cache holds B; scratch and bounds are allocated
            oa, ob = Out(ctx, 3, nfft, 7), Out(ctx, 3, nfft, 7)
            try:
                probe = hog.start()
                assert hog.busy(probe), 'the hog is too short'
                oa.launch(d, sb, thr, *A)
                ob.launch(d, sb, thr, *B)
                hog.finish(probe)
                ctx.sync()
                bit_equal(oa.read(), want_a)
                bit_equal(ob.read(), want_b)
            finally:
                oa.free()
                ob.free()
    finally:
        hog.close()


# ---- 4. hard rows ---------------------------------------------------------------------------------------------------

def through_everything(ctx, rows, sb, thr, lo, hi, ref, floor=0.0, label=None):
    """Both decision entry points, oth_bin_threshold and oth_channel_power on the same rows against one reference."""
    e = check(both_entries(ctx, rows, sb, thr, lo, hi), ref, lo, hi, floor, thr)
    m, n = ctx.bin_threshold(rows, sb, thr)
    eb = check((m, n, None), ref, floor=floor, thr=thr)
    ec = 0.0
    for i, row in enumerate(rows):
        p, ma = ctx.channel_power(row, sb, lo, hi, want_movavg=True)
        one = ref.head(i + 1)
        one.rows, one.ma, one.noise, one.power = one.rows[i:], one.ma[i:], one.noise[i:], one.power[i:]
        with np.errstate(over='ignore', invalid='ignore'):
            ma32 = one.ma[0].astype(np.float32)
            wild = ~np.isfinite(ma32)
            assert np.array_equal(ma[wild], ma32[wild], equal_nan=True)
            ok = np.abs(ma - one.ma[0]) <= S.RTOL_POWER * one.ma[0] + floor
        assert np.all(ok | wild), (i, np.flatnonzero(~(ok | wild))[:8])
        ec = max(ec, check((None, np.array([one.noise[0]], np.float32), p[None, :]), one, lo, hi, floor)[1])
    if label:
        print('scan-err %s decide: noise %.3g power %.3g; bin_threshold: noise %.3g; channel_power: %.3g'
              % (label, e[0], e[1], eb[0], ec))


def carrier_rows(nfft, M, seed):
    """A floor of 1e-12 (+ 10 %) with carriers 100 / 130 / 150 dB above it on run, block and tile edges and in pairs
    exactly M and M - 1 bins apart."""
    rng = np.random.default_rng(seed)
    at = [0, 7, 8, 4095, 4096, 4097, nfft - 1, 1500, 1500 + M, 2700, 2700 + M - 1]
    if nfft > 17000:
        at += [8191, 8192, 16384, 12000, 12000 + M, 12288 - M + 1, 12288]
    rows = np.empty((3, nfft), np.float32)
    for i, db in enumerate((100.0, 130.0, 150.0)):
        row = 1e-12 * (1.0 + 0.1 * rng.random(nfft))
        row[at] = 1e-12 * 10.0 ** (db / 10.0)
        rows[i] = row.astype(np.float32)
    return rows


@pytest.mark.parametrize('nfft', [4104, 20000])
@pytest.mark.parametrize('sb', [9.0, 163.84, 1024.5])
def test_carriers_next_to_the_floor(ctx, nfft, sb):
    """The sliding sum must not carry a carrier's rounding into the floor beside it, wherever the carrier sits in a
    run, a block of 8 or a tile.  Reference: every window summed exactly."""
    rows = carrier_rows(nfft, int(sb), nfft + int(sb))
    lo, hi = S.even_slices(nfft, 16)
    ref = S.Ref(rows, sb, 3.0, lo, hi, exact=True)
    assert all(0 < int(m.sum()) < 40 for m in ref.mask)
    through_everything(ctx, rows, sb, 3.0, lo, hi, ref, label='carriers n%d sb%s' % (nfft, sb))


@pytest.mark.parametrize('nfft', [4104, 20000, 4099])
@pytest.mark.parametrize('sb', [9.0, 163.84])
def test_mixed_sign_rows(ctx, nfft, sb):
    """The moving average is the abs of a sum that cancels.  On top of the relative tolerance every output gets an
    absolute floor of 2^-24 max|row|: the rows are float32, so one rounding of the largest input is the smallest
    error a window sum can be said to carry, and a window whose sum cancels below that has no digits to compare."""
    rng = np.random.default_rng(nfft + int(sb))
    rows = rng.standard_normal((3, nfft)).astype(np.float32)
    floor = 2.0 ** -24 * float(np.abs(rows).max())
    lo, hi = S.even_slices(nfft, 16)
    ref = S.Ref(rows, sb, 3.0, lo, hi, exact=True)
    through_everything(ctx, rows, sb, 3.0, lo, hi, ref, floor=floor, label='mixed-sign n%d sb%s' % (nfft, sb))


@pytest.mark.parametrize('nfft', [4104, 4099])
def test_zero_rows(ctx, nfft):
    rows = np.zeros((3, nfft), np.float32)
    rows[1, 2000] = 1.0
    rows[2, 4096] = 1.0
    lo, hi = S.even_slices(nfft, 16)
    ref = S.Ref(rows, 163.84, 3.0, lo, hi, exact=True)
    assert np.all(ref.noise == 0) and ref.mask.sum() == 2
    through_everything(ctx, rows, 163.84, 3.0, lo, hi, ref)


@pytest.mark.parametrize('nfft', [4104, 4099])
def test_denormal_rows(ctx, nfft):
    """float32 denormals (1e-40) are inputs like any other: a library built to flush them gives a zero noise floor.
    With M = srch_bins = 8 and bins that are q or 64 q every window sum and its eighth are exact in double."""
    q = np.float32(1e-40)
    assert 0 < q < np.finfo(np.float32).tiny
    rng = np.random.default_rng(nfft)
    rows = np.full((3, nfft), q, np.float32)
    rows[rng.random((3, nfft)) < 0.02] = q * np.float32(64)
    lo, hi = S.even_slices(nfft, 16)
    ref = S.Ref(rows, 8.0, 3.0, lo, hi, exact=True)
    assert np.all(ref.noise > 0) and np.all(ref.power > 0)
    got = both_entries(ctx, rows, 8.0, 3.0, lo, hi)
    assert np.all(got[1] > 0) and np.all(got[2] > 0)
    through_everything(ctx, rows, 8.0, 3.0, lo, hi, ref)


@pytest.mark.parametrize('nfft', [4104, 4099])
@pytest.mark.parametrize('thr', [1.5, 10.0])
def test_rows_near_float32_max(ctx, nfft, thr):
    """Bins of 2 ... 2.5e38: a float32 sum of 163 of them overflows, the double sums do not; a channel sum over two or
    more bins rounds to inf in float32 exactly where the reference's does, and thr = 10 puts the level at inf."""
    rng = np.random.default_rng(nfft)
    rows = (2.5e38 * (0.8 + 0.2 * rng.random((3, nfft)))).astype(np.float32)
    sl = [(5, 6), (nfft - 1, nfft), (2000, 2001), (2000, 2002), (0, nfft), (7, 7), (3000, 3010)]
    lo, hi = np.array([a for a, _ in sl], np.int32), np.array([b for _, b in sl], np.int32)
    ref = S.Ref(rows, 163.84, thr, lo, hi)
    with np.errstate(over='ignore'):
        p32 = ref.power.astype(np.float32)
    assert np.all(np.isfinite(ref.ma)) and np.all(np.isfinite(p32[:, :3])) and np.all(np.isinf(p32[:, [3, 4, 6]]))
    assert np.isinf(ref.level).all() == (thr == 10.0)
    through_everything(ctx, rows, 163.84, thr, lo, hi, ref)


# ---- 5. non-finite bins, NaN and the noise floor, windows longer than the row ------------------------------------------

@pytest.mark.parametrize('nfft', [4100, 20000, 4099])
@pytest.mark.parametrize('value', [np.inf, -np.inf, np.nan])
def test_a_non_finite_bin_leaves_with_its_window(ctx, nfft, value):
    """np.convolve gives non-finite outputs in exactly the M windows that hold the bin.  One-bin channel slices show
    every moving-average output of the decision stage: non-finite where the reference's are and nowhere else, and the
    finite ones right (a sliding sum keeps inf - inf = NaN to the end of its run unless it starts again)."""
    sb, thr = 163.84, 3.0
    rows = S.gamma_rows(2, nfft, 81 + nfft)
    inside = np.zeros(nfft, bool)
    for k in (2000, 3 * nfft // 4 + 5, 4093 if nfft > 4300 else 4010, nfft - 3):      # (4010 + 81 = 4091: to the end of a run)
        rows[0, k] = value
        inside[max(0, k - 81):k + 82] = True                # M = 163: bin k is a tap of outputs k - 81 ... k + 81
    lo = np.arange(nfft, dtype=np.int32)
    hi = lo + 1
    ref = S.Ref(rows, sb, thr, lo, hi)
    assert np.array_equal(~np.isfinite(ref.ma[0]), inside) and np.isfinite(ref.ma[1]).all()
    got = both_entries(ctx, rows, sb, thr, lo, hi)
    assert np.array_equal(np.isfinite(got[2]), np.isfinite(ref.ma)), \
        np.flatnonzero(np.isfinite(got[2][0]) != np.isfinite(ref.ma[0]))[:16]
    check(got, ref, lo, hi)
    p, ma = ctx.channel_power(rows[0], sb, lo[:8], hi[:8], want_movavg=True)
    assert np.array_equal(np.isfinite(ma), np.isfinite(ref.ma[0]))


@pytest.mark.parametrize('nfft', [4100, 20000, 4099])
def test_a_nan_bin_makes_the_noise_floor_nan(ctx, nfft):
    """numpy's min keeps a NaN: the row's noise floor is NaN and its mask empty (the reference's movingaverage(...).min()
    and np.amin); the other rows of the call are untouched.  Through oth_bin_threshold and both doors of the decision
    stage, with the NaN in the last tile."""
    sb, thr = 9.0, 3.0
    clean = S.gamma_rows(5, nfft, 91 + nfft)
    rows = clean.copy()
    rows[2, nfft - 700] = np.nan
    lo, hi = S.even_slices(nfft, 5)
    ref = S.Ref(rows, sb, thr, lo, hi)
    assert np.isnan(ref.noise[2]) and not ref.mask[2].any() and np.isfinite(ref.noise[[0, 1, 3, 4]]).all()
    got, was = both_entries(ctx, rows, sb, thr, lo, hi), both_entries(ctx, clean, sb, thr, lo, hi)
    check(got, ref, lo, hi)
    keep = [0, 1, 3, 4]
    bit_equal((got[0][keep], got[1][keep], got[2][keep]), (was[0][keep], was[1][keep], was[2][keep]))
    m, n = ctx.bin_threshold(rows, sb, thr)
    m0, n0 = ctx.bin_threshold(clean, sb, thr)
    check((m, n, None), ref)
    assert np.isnan(n[2]) and not m[2].any()
    assert np.array_equal(m[keep], m0[keep]) and np.array_equal(n[keep], n0[keep])


@pytest.mark.parametrize('nfft,sb', [(64, 100.0), (4, 5.0), (64, 65.0), (4100, 1e12)])
def test_a_window_longer_than_the_row_is_refused(ctx, nfft, sb):
    """With int(srch_bins) > nfft np.convolve swaps its arguments and the reference's movingaverage returns
    int(srch_bins) values (oracle.ref_cpu.movingaverage(ones(64), 100.0) has 100): no nfft-long answer is that one,
    so every entry point that takes srch_bins refuses, and so do the helpers of ofdm_cr_tools built on them."""
    from ofdm_tools import ofdm_cr_tools as T
    if sb < 1e6:
        assert len(R.movingaverage(np.ones(nfft), sb)) == int(sb) != nfft
    rows = S.gamma_rows(2, nfft, 3)
    with DevRows(ctx, rows) as d:
        o = Out(ctx, 2, nfft, 1)
        try:
            refused(ctx, lambda: ctx.scan_decide_dev(d.ptr, 2, nfft, sb, 3.0, [0], [1]), 'nfft')
            refused(ctx, lambda: ctx.scan_decide_dev(d.ptr, 2, nfft, sb, 3.0), 'nfft')
            refused(ctx, lambda: ctx.scan_decide_dev_out(d.ptr, 2, nfft, sb, 3.0, [0], [1], o.ptrs[1], o.ptrs[2],
                                                         o.ptrs[0]), 'nfft')
        finally:
            o.free()
    refused(ctx, lambda: ctx.bin_threshold(rows, sb, 3.0), 'nfft')
    refused(ctx, lambda: ctx.channel_power(rows[0], sb, [0], [1]), 'nfft')
    refused(ctx, lambda: T.movingaverage(rows[0], sb, ctx), 'nfft')
    Sf = 64000
    refused(ctx, lambda: T.src_power(rows[0], nfft, float(Sf) / nfft, Sf, T.frange(-Sf // 2, Sf // 2, 8000), sb, ctx), 'nfft')


@pytest.mark.parametrize('nfft,sb', [(64, 64.0), (64, 64.9), (4, 4.0), (4, 4.5), (1021, 1021.0), (1024, 1024.0)])
def test_a_window_as_long_as_the_row(ctx, nfft, sb):
    from ofdm_tools import ofdm_cr_tools as T
    assert len(R.movingaverage(np.ones(nfft), sb)) == nfft
    rows = S.gamma_rows(3, nfft, 7 + nfft)
    lo, hi = S.even_slices(nfft, min(4, nfft))
    ref = S.Ref(rows, sb, 1.5, lo, hi)
    through_everything(ctx, rows, sb, 1.5, lo, hi, ref)
    assert S.relerr(T.movingaverage(rows[0], sb, ctx), ref.ma[0]) <= S.RTOL_POWER


# ---- 6. the host-row small ops -----------------------------------------------------------------------------------------

HOST_SHAPES = [(n, sb) for n, sb in SHAPES if n <= 20000 and n * int(sb) <= 2.1e7]


@pytest.mark.parametrize('nfft,sb', HOST_SHAPES, ids=['n%d-sb%s' % c for c in HOST_SHAPES])
def test_channel_power_shapes(ctx, nfft, sb):
    row = S.gamma_rows(1, nfft, 2000 * nfft + int(100 * sb))
    lo, hi = S.even_slices(nfft, min(nfft, 7))
    ref = S.Ref(row, sb, 3.0, lo, hi)
    p, ma = ctx.channel_power(row[0], sb, lo, hi, want_movavg=True)
    assert ma.shape == (nfft,) and S.relerr(ma, ref.ma[0]) <= S.RTOL_POWER, S.relerr(ma, ref.ma[0])
    assert np.array_equal(p, ctx.channel_power(row[0], sb, lo, hi))
    e = check((None, ref.noise, p[None, :]), ref, lo, hi)
    print('scan-err channel_power n%d sb%s movavg %.3g power %.3g' % (nfft, sb, S.relerr(ma, ref.ma[0]), e[1]))


@pytest.mark.parametrize('nfft,sb', HOST_SHAPES, ids=['n%d-sb%s' % c for c in HOST_SHAPES])
def test_bin_threshold_shapes_and_the_decision_stage_agree(ctx, nfft, sb):
    """oth_bin_threshold on 300, 5 or 1 rows (by the cost of the float64 reference) against the reference, and against
    the decision stage on the same rows: one divides by srch_bins, the other multiplies by its reciprocal, so the two
    noise floors are held to the tolerance, not to equal bits."""
    work = nfft * int(sb)
    nrows = 300 if work <= 2e5 else 5 if work <= 4e6 else 1
    thr = thr_of(nfft, sb)
    rows = S.gamma_rows(nrows, nfft, 3000 * nfft + int(100 * sb))
    ref = S.Ref(rows, sb, thr)
    m, n = ctx.bin_threshold(rows, sb, thr)
    e = check((m, n, None), ref)
    with DevRows(ctx, rows) as d:
        dm, dn, _ = ctx.scan_decide_dev(d.ptr, nrows, nfft, sb, thr)
    assert np.allclose(n, dn, rtol=S.RTOL_NOISE, atol=0), S.relerr(n, dn)
    masks_agree(m, dm, ref)
    print('scan-err bin_threshold n%d sb%s rows %d noise %.3g' % (nfft, sb, nrows, e[0]))


@pytest.mark.parametrize('nfft', [1, 63, 1000, 4099, 16384])
@pytest.mark.parametrize('group', [1, 2, 3, 8, 128, 'nrows'])
def test_rows_group_mean(ctx, nfft, group):
    """Trailing rows that do not fill a group are dropped; rows 100 dB apart inside a group.  rtol 2^-23: the sum is
    taken in double, the result is rounded to float32 once (2^-24), and the float64 mean it is compared with is exact
    to 2^-50."""
    g = 7 if group == 'nrows' else group
    nrows = g if group == 'nrows' else 3 * g + (g - 1 if g > 1 else 0)
    rng = np.random.default_rng(1000 * nfft + g)
    rows = (rng.gamma(4.0, 0.25, (nrows, nfft)) * 10.0 ** rng.uniform(-10.0, 0.0, (nrows, 1))).astype(np.float32)
    got = ctx.rows_group_mean(rows, g)
    ref = rows[:nrows // g * g].astype(np.float64).reshape(-1, g, nfft).mean(1)
    assert got.shape == ref.shape and S.relerr(got, ref) <= 2.0 ** -23, S.relerr(got, ref)


def test_rows_group_mean_refusals(ctx):
    import ctypes as C
    rows = np.ones((3, 64), np.float32)
    out = np.zeros((3, 64), np.float32)
    fp = C.POINTER(C.c_float)
    for nrows, group in ((3, 4), (3, 0), (3, -1), (0, 1)):
        rc = ctx.lib.oth_rows_group_mean(ctx.h, rows.ctypes.data_as(fp), nrows, 64, group, out.ctypes.data_as(fp))
        assert rc == ERR_INVALID and ctx.lib.oth_last_error(ctx.h), (nrows, group, rc)
    assert np.array_equal(ctx.rows_group_mean(rows, 3), np.ones((1, 64), np.float32))


def test_70000_rows(ctx):
    """The row index of the decision stage is gridDim.y, which a runtime may limit: 70000 rows of 64 bins are either
    right or refused with a message, and the context works afterwards (right on ROCm's HIP, which takes 2^32 - 1 threads
    per grid dimension)."""
    from ofdm_tools._hip import HipError
    nrows, nfft, sb, thr = 70000, 64, 9.0, 3.0
    rows = S.gamma_rows(nrows, nfft, 70000)
    lo, hi = S.even_slices(nfft, 3)
    pick = np.r_[0:40, 65500:65600, nrows - 40:nrows, np.random.default_rng(1).integers(0, nrows, 200)]
    ref = S.Ref(rows[pick], sb, thr, lo, hi)
    with DevRows(ctx, rows) as d:
        try:
            host = ctx.scan_decide_dev(d.ptr, nrows, nfft, sb, thr, lo, hi)
            out = dev_out(ctx, d, sb, thr, lo, hi)
        except HipError as e:
            assert e.code in (ERR_INVALID, ERR_HIP) and str(e).split('):', 1)[1].strip()
            print('70000 rows refused: %s' % e)
        else:
            bit_equal(host, out)
            check((host[0][pick], host[1][pick], host[2][pick]), ref, lo, hi)
    small = S.gamma_rows(3, 4100, 5)
    l5, h5 = S.even_slices(4100, 5)
    check(both_entries(ctx, small, 163.84, thr, l5, h5), S.Ref(small, 163.84, thr, l5, h5), l5, h5)


def test_70000_groups(ctx):
    from ofdm_tools._hip import HipError
    ngroups, nfft, g = 70000, 64, 2
    rng = np.random.default_rng(70001)
    rows = (rng.gamma(4.0, 0.25, (ngroups * g, nfft)) * 10.0 ** rng.uniform(-10.0, 0.0, (ngroups * g, 1))).astype(np.float32)
    try:
        got = ctx.rows_group_mean(rows, g)
    except HipError as e:
        assert e.code in (ERR_INVALID, ERR_HIP) and str(e).split('):', 1)[1].strip()
        print('70000 groups refused: %s' % e)
    else:
        ref = rows.astype(np.float64).reshape(-1, g, nfft).mean(1)
        assert got.shape == ref.shape and S.relerr(got, ref) <= 2.0 ** -23
    assert np.array_equal(ctx.rows_group_mean(np.ones((4, 8), np.float32), 2), np.ones((2, 8), np.float32))


# ---- 7. through the block ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,trunc_band', [(1000, None), (4099, None), (20000, 800000), (65536, None)])
def test_batch_scan_plan_decide_at_any_length(ctx, N, trunc_band):
    """BatchScanPlan.decide() on host rows against the oracle's ScannerState + src_power: the slice bounds the block
    computes (with a truncated band in one case) and the any-length row lengths meet the decision stage."""
    from ofdm_tools.scan_batch import BatchScanPlan
    Sf, cs, bw, thr = 1000000, 15625.0, 10e3, 3.0
    tb = Sf if trunc_band is None else trunc_band
    bp = BatchScanPlan(ctx, N, Sf, cs, bw, thr_leveler=thr, trunc_band=tb)
    st = R.ScannerState(N, Sf, cs, bw, trunc_band=tb)
    assert bp.scanner.srch_bins == st.srch_bins and (st.trunc > 0) == (trunc_band is not None)
    rows = S.gamma_rows(3, N, 11 + N)
    mask, noise, plc = bp.decide(rows)
    want = []
    for row in rows:
        w = R.src_power(row.astype(np.float64), N, st.Fr, Sf, st.bb_freqs, st.srch_bins)
        want.append(w[st.trunc_ch:-st.trunc_ch] if st.trunc > 0 else w)
    want = np.array(want)
    assert plc.shape == want.shape == (3, len(st.ax_ch))
    ref = S.Ref(rows, st.srch_bins, thr)
    ref.power = want
    e = check((mask, noise, plc), ref)
    assert any(0 < int(m.sum()) < N for m in ref.mask)
    print('scan-err block N%d noise %.3g power %.3g' % (N, e[0], e[1]))
    bp.plan.close()
