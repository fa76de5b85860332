"""GPU tests of the block classes (same names / constructor signatures as the reference) against
the CPU oracle: the whole chain from complex64 stream to decisions, messages and PDUs."""
import os
import struct

import numpy as np
import pytest

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.fixture(scope='module')
def ctx():
    from ofdm_tools import _hip
    c = _hip.Context(0)
    yield c
    c.close()


def test_spectrum_sensor_v2_state_sequence(ctx, golden, tmp_path):
    import ofdm_tools
    g = golden('scanner_state_seq.npz')
    subj = list(g['subject_channels'])
    blk = ofdm_tools.spectrum_sensor_v2(1024, 1000, 1000000, channel_space=25e3, search_bw=12.5e3, thr_leveler=4,
                                        tune_freq=100000000, alpha_avg=0.5, trunc_band=800000, stats=True, psd=True,
                                        output='o', subject_channels=subj, ctx=ctx, threaded=False, log_directory=str(tmp_path))
    assert blk.decimation == 1 and np.allclose(blk.ax_ch, g['ax_ch'])
    msgs = []
    for i in range(4):
        blk.msg_connect('freq_out_%d' % i, lambda m, i=i: msgs.append((i, m)))
    x = g['x']
    for i in range(16):                                   # one vector per work() call, like one message each
        assert blk.work([x[i * 1024:(i + 1) * 1024]], []) == 1024
        assert np.allclose(blk.power_level_ch, g['plc_seq'][i], rtol=1e-4)
        assert np.isclose(blk.noise_estimate, g['noise_seq'][i], rtol=1e-4)
        occ = [1.0 if a in blk.spectrum_constraint_hz else 0.0 for a in blk.ax_ch]
        assert occ == list(g['occupied_seq'][i])
    assert np.allclose(blk._logger.cumulative_max_power, g['cumulative_max'], rtol=1e-4)
    assert relerr(blk._logger.cumulative_psd, g['peak']) < RTOL
    assert blk.top4 == list(g['top4'])
    last = {i: m for i, m in msgs}
    assert [last[i][1] for i in range(4)] == [f - 100000000 for f in g['top4']]
    files = blk._logger.flush()
    assert relerr(np.load(files['psd']), g['peak']) < RTOL
    assert 'statistics ' + str(blk._logger.cumulative_statistics) in open(files['stat']).read()


def test_spectrum_sensor_v1_is_the_stats_path(ctx, golden, tmp_path):
    import ofdm_tools
    g = golden('scanner_state_seq.npz')
    blk = ofdm_tools.spectrum_sensor_v1(1024, 1000, 1000000, channel_space=25e3, search_bw=12.5e3, thr_leveler=4,
                                        tune_freq=100000000, alpha_avg=0.5, trunc_band=800000, psd=True, ctx=ctx, threaded=False,
                                        log_directory=str(tmp_path))
    blk.feed(g['x'], max_items=1024)
    assert np.isclose(blk.noise_estimate, g['noise_seq'][-1], rtol=1e-4)
    assert np.allclose(blk._logger.cumulative_max_power, g['cumulative_max'], rtol=1e-4)
    assert relerr(blk._logger.cumulative_psd, g['peak']) < RTOL
    # what v1 does not have (python/spectrum_sensor_v1.py:40-104): message ports, strobes, the smoothed copy, set_freqs
    assert blk.name() == 'spectrum_sensor_v1' and blk._strobes == []
    assert not any(p.startswith('freq_') for p in blk._out_ports)
    assert not np.any(blk.power_level_ch)
    with pytest.raises(AttributeError):
        blk.set_freqs(1, 2, 3, 4)


def test_spectrum_sensor_v2_decimation_and_scheduler_chunks(ctx):
    import ofdm_tools
    fft_len, Sf = 256, 256 * 100
    blk = ofdm_tools.spectrum_sensor_v2(fft_len, 20, Sf, channel_space=1600, search_bw=800, trunc_band=Sf - 3200,
                                        stats=True, ctx=ctx, threaded=False)
    assert blk.decimation == 5                             # int(25600/256/20), keep_one_in_n(5)
    x = R.synth_iq(fft_len * 40 + 13, 17)
    assert blk.feed(x, max_items=1000) == len(x)           # ragged scheduler chunks
    rows = R.chain_sensor_v2(x, fft_len, decim=5)
    st = R.ScannerState(fft_len, Sf, 1600, 800, trunc_band=Sf - 3200)
    # the watcher sees the last kept vector of each work() call; with 1000-sample calls no call
    # completes two kept vectors, so every row is seen
    for r in rows:
        st.scan(r.astype(np.float32))
    assert np.allclose(blk.power_level_ch, st.plc, rtol=1e-4)
    assert blk._scanner.n_measurements == len(rows) == 8


def test_multichannel_scanner_top4(ctx):
    import ofdm_tools
    fft_len, Sf = 16384, 1000000
    st = R.ScannerState(fft_len, Sf, 15625.0, 10e3, tune_freq=0, trunc_band=Sf)     # trunc = 0: all 64 channels
    subj = [st.ax_ch[i] for i in (5, 12, 20, 33, 40, 51)]
    blk = ofdm_tools.multichannel_scanner(fft_len, 1000, Sf, channel_space=15625.0, search_bw=10e3, tune_freq=0,
                                          trunc_band=Sf, subject_channels=subj, ctx=ctx, threaded=False)
    x = R.synth_iq(fft_len * 3, 3000)
    dec = blk.decimation
    assert dec == 1
    blk.feed(x, max_items=fft_len)
    rows = R.chain_sensor_v2(x, fft_len, decim=dec)
    for r in rows:
        st.scan(r.astype(np.float32))
    assert np.allclose(blk.power_level_ch, st.plc, rtol=1e-4)
    pwr, best = R.publish_top4(st.plc, st.ax_ch, subj)
    assert blk.top4 == best and np.allclose(blk.subject_channels_pwr, pwr, atol=1e-3)


def test_psd_logger_peak_file(ctx, golden, tmp_path):
    import ofdm_tools
    g = golden('gr_chain_bh_mag_peak_4096.npz')
    path = str(tmp_path / 'psd_log.npy')
    blk = ofdm_tools.psd_logger(4096, 1000, 4096 * 1000, ctx=ctx, threaded=False, mat_file=path)
    assert blk.decimation == 1
    saves, inner = [], blk._on_vector
    blk._on_vector = lambda row: (inner(row), saves.append(np.load(path)))
    blk.feed(g['x'], max_items=4096)
    assert relerr(blk.peak_vals, g['expected_peak'][-1]) < RTOL
    assert relerr(np.load(path), g['expected_peak'][-1]) < RTOL
    # every file the reference's OWN watcher body saved for these vectors (psd_logger.py:70-88 on stand-in messages,
    # ref_psd_logger.npz): one save per vector, the first vector is the first peak
    ref = golden('ref_psd_logger.npz')
    assert len(saves) == len(ref['saved_peaks']) == 16
    for got, want in zip(saves, ref['saved_peaks']):
        assert got.dtype == want.dtype == np.float32 and relerr(got, want) < RTOL


def test_local_worker_pdus(ctx, golden):
    import ofdm_tools
    from ofdm_tools import packets
    g = golden('gr_chain_bh_iir_log_2048.npz')
    N, Sf, alpha = 2048, int(g['sample_rate']), float(g['average'])
    blk = ofdm_tools.local_worker(N, Sf, alpha, Sf / N, 1472, True, ctx=ctx, threaded=False)   # rate = one PSD per vector
    frames = []
    blk.msg_connect('pdus', lambda m: frames.append(m[1]))
    x = g['x']
    blk.work([x[:N]], [])
    assert len(frames) == 6 and frames[0][0] == 6                              # ceil(8192/1470)
    db0 = np.frombuffer(packets.reassemble(frames), '<f4')
    k = -10 * np.log10(N) - 10 * np.log10(Sf)
    assert relerr(10 ** ((db0.astype(np.float64) - k) / 10), g['expected_lin'][0]) < RTOL
    blk.feed(x[N:], max_items=N)
    assert relerr(10 ** ((blk.last_db.astype(np.float64) - k) / 10), g['expected_lin'][-1]) < RTOL
    assert frames[-6:] == R.worker_fragments(blk.last_db, 1470, N, True)
    # 8-bit mode: int8 cast of the dB values, ceil(2048/1470) = 2 frames
    blk.set_data_precision(False)
    del frames[:]
    blk.send_packet(blk.last_db)
    assert frames == R.worker_fragments(blk.last_db, 1470, N, False) and len(frames) == 2


class FakeReceiver(object):
    def __init__(self):
        self.tuned = []

    def set_center_freq(self, f, chan):
        self.tuned.append(f)


def test_spectrum_sweeper_sweep_and_wire_format(ctx):
    import ofdm_tools
    from ofdm_tools import packets
    rx = FakeReceiver()
    fft_len, Sf, tSf = 4096, 2000000, 1750000
    blk = ofdm_tools.spectrum_sweeper(rx, 'rtl', fft_len, Sf, tSf, 100e6, 107e6, 15, 0.0, 8, 0, 1472, ctx=ctx,
                                      threaded=False)
    pts, tune, excess = R.sweeper_geometry(fft_len, Sf, tSf, 100e6, 107e6, 8)
    assert (blk.vector_probe_pts, blk.tune_frequencies, blk.excess_bins) == (pts, tune, excess) == (16384, tune, 256)
    assert len(tune) == 4
    vectors = [R.synth_iq(pts, 2000 + i) for i in range(len(tune))]
    it = iter(vectors)
    blk.get_samples = lambda: next(it)                    # what data_colector would have stored after each retune
    frames = []
    blk.msg_connect('pdus', lambda m: frames.append(m[1]))
    psd = blk.sweep_once(sleep=lambda s: None)
    ref = R.sweeper_stitch(vectors, fft_len, Sf, excess, 0.0)
    assert rx.tuned == tune and psd.shape == ref.shape == (4 * 3584,)
    assert relerr(10 ** (psd / 10), 10 ** (ref / 10)) < RTOL
    payload = packets.reassemble(frames)
    assert np.allclose(np.frombuffer(payload, '<f4'), psd.astype(np.float32))
    assert frames == R.sweeper_fragments(struct.pack('<%df' % len(psd), *psd), 1470)
    # the sharded sweep (one process here: rank 0 of 1) gives the same wideband PSD
    import torch
    dev = torch.device('cuda', 0)
    wide = blk.sweep_once_sharded(lambda i, f: vectors[i], 0, 1, dev)
    assert np.allclose(wide, psd, rtol=1e-6)
    # captures that are already device tensors (complex64) take the same path without the upload
    tv = [torch.from_numpy(v).to(dev) for v in vectors]
    wide = blk.sweep_once_sharded(lambda i, f: tv[i], 0, 1, dev)
    assert np.allclose(wide, psd, rtol=1e-6)
    # flowgraph side: work() keeps the last complete capture
    blk2 = ofdm_tools.spectrum_sweeper(rx, 'rtl', fft_len, Sf, tSf, 100e6, 107e6, 1e9, 0.0, 8, 0, 1472, ctx=ctx,
                                       threaded=False)
    x = R.synth_iq(pts * 2 + 100, 5)
    blk2.feed(x, max_items=5000)
    assert np.array_equal(blk2.get_samples(), x[pts:2 * pts])


def test_ref_stitcher_pass_through_the_block(ctx, golden):
    """a5 against the reference's OWN spectrum_stitcher.run (spectrum_sweeper.py:207-231, ref_threads.npz): the same
    three captures through the block - retune order on channel 0, the tune delay after every retune, concatenation,
    the blend with the 1e-10 floor, little-endian float32 payload, the sweeper's framing."""
    import ofdm_tools
    from ofdm_tools import packets
    g = golden('ref_threads.npz')
    nfft, fs, ex = int(g['stitch_nfft']), int(g['stitch_fs']), int(g['stitch_excess'])
    freqs = [float(f) for f in g['stitch_freqs']]
    tSf = fs - 2 * ex * fs // nfft                       # excess_bins = floor((Sf - tSf) / 2 / (Sf / fft_len)) = 96
    rx = FakeReceiver()
    tuned = []
    rx.set_center_freq = lambda f, chan: tuned.append([f, float(chan)])
    blk = ofdm_tools.spectrum_sweeper(rx, 'rtl', nfft, fs, tSf, freqs[0] - tSf / 2, freqs[-1] + tSf / 2, 15,
                                      float(g['stitch_average']), 8, 125, 1472, ctx=ctx, threaded=False)
    assert blk.excess_bins == ex and blk.get_tune_delay() == 0.125
    blk.tune_frequencies = freqs
    it = iter(list(g['stitch_captures']))
    blk.get_samples = lambda: next(it)
    frames, sleeps = [], []
    blk.msg_connect('pdus', lambda m: frames.append(m[1]))
    psd = blk.sweep_once(sleep=sleeps.append)
    assert tuned == g['stitch_tuned'].tolist() and sleeps == g['stitch_sleeps'].tolist()[1:]
    want = np.frombuffer(bytes(g['stitch_packed']), '<f4').astype(np.float64)
    got = np.frombuffer(packets.reassemble(frames), '<f4').astype(np.float64)
    assert got.shape == want.shape == psd.shape
    # the reference's Welch ran in SciPy's single precision (complex64 in), 2e-5 off the float64 oracle itself
    assert relerr(10 ** (got / 10), 10 ** (want / 10)) < RTOL + 2e-5
    assert [f[:2] for f in frames] == [f[:2] for f in R.sweeper_fragments(bytes(g['stitch_packed']), 1470)]
    assert [len(f) for f in frames] == [len(f) for f in R.sweeper_fragments(bytes(g['stitch_packed']), 1470)]


def test_ref_watchers_through_the_blocks(ctx, golden, tmp_path):
    """a10 / a15 against the reference's OWN watcher bodies (psd_watcher.run, waterfall_watcher.run,
    spectrum_sensor_v2.py:304-354; main_thread.run, local_worker.py:126-139): work() calls of 1, 3, 1, 2, 1, 4, 1, 3
    vectors stand for the messages - the last vector of each is the one that counts; the PSD peak is the running
    maximum of those, the waterfall their sequence, local_worker's PDUs carry them."""
    import ofdm_tools
    from ofdm_tools import packets
    from test_hip_parity import check_single_rows
    g = golden('ref_threads.npz')
    c = golden(str(g['input_from']))
    N = 1024
    x = c['x'].astype(np.complex64)
    edges = np.concatenate(([0], np.cumsum(g['msg_counts']))) * N
    blk = ofdm_tools.spectrum_sensor_v2(N, 1, N, psd=True, waterfall=True, ctx=ctx, threaded=False,
                                        log_directory=str(tmp_path))
    assert blk.decimation == 1
    for a, b in zip(edges[:-1], edges[1:]):
        assert blk.work([x[a:b]], []) == b - a
    rows = np.array(blk._logger.cumulative_waterfall)
    assert rows.shape == g['waterfall'].shape
    check_single_rows(rows, g['waterfall'].astype(np.float64))
    check_single_rows(blk._logger.cumulative_psd[None, :], g['psd_cumulative'][None, :].astype(np.float64))
    check_single_rows(blk._logger.periodic_psd_peaks[None, :], g['psd_periodic_peaks'][None, :].astype(np.float64))
    blk.stop()


def test_spectrum_sweeper_stitcher_thread_sweeps_by_itself(ctx):
    """spectrum_sweeper.py:99-105,207-231: constructing the block starts the stitcher; a flowgraph only feeds work().
    Nothing here calls sweep_once."""
    import time
    import ofdm_tools
    from ofdm_tools import packets
    rx = FakeReceiver()
    fft_len, Sf, tSf = 1024, 2000000, 1750000
    blk = ofdm_tools.spectrum_sweeper(rx, 'rtl', fft_len, Sf, tSf, 100e6, 107e6, 1e9, 0.0, 4, 2, 1472, ctx=ctx,
                                      start_delay=0.05)
    pts, tune, excess = R.sweeper_geometry(fft_len, Sf, tSf, 100e6, 107e6, 4)
    nbins = fft_len - 2 * excess
    frames = []
    blk.msg_connect('pdus', lambda m: frames.append(m[1]))
    x = R.synth_iq(pts, 77)
    end = time.monotonic() + 20
    while blk.sweeps_done < 3 and time.monotonic() < end:
        blk.feed(x, max_items=4096)              # the scheduler thread: the same capture over and over
        time.sleep(0.002)
    assert blk.sweeps_done >= 3
    blk.set_tune_delay(1)                        # reaches the running stitcher (:110-112)
    assert blk.get_tune_delay() == 1e-3
    blk.stop()
    assert blk._stitch_thread is None
    n_tuned, n_frames = len(rx.tuned), len(frames)
    time.sleep(0.05)
    assert (len(rx.tuned), len(frames)) == (n_tuned, n_frames)          # really stopped
    k = len(tune)
    assert rx.tuned[:3 * k] == tune * 3
    per_sweep = packets.sweeper_fragment_count(4 * k * nbins, 1470)
    assert len(frames) >= 3 * per_sweep
    payload = packets.reassemble(frames[:per_sweep])
    got = np.frombuffer(payload, '<f4').astype(np.float64)
    # every segment of the first sweep saw either the initial 1e-10 vector (:84) or the capture x
    ref_x = R.sweeper_src_power(x, fft_len, Sf, excess)
    with np.errstate(divide='ignore'):      # the reference's initial vector is a constant: detrended to zero, -inf dB (spectrum_sweeper.py:84)
        ref_0 = R.sweeper_src_power(np.array([1e-10] * pts, np.complex64), fft_len, Sf, excess)
    assert got.shape == (k * nbins,)
    for j in range(k):
        seg = got[j * nbins:(j + 1) * nbins]
        ok_x = relerr(10 ** (seg / 10), 10 ** (ref_x / 10)) < RTOL
        assert ok_x or np.allclose(seg, ref_0, atol=1e-3) or not np.all(np.isfinite(ref_0))
    last = np.frombuffer(packets.reassemble(frames[2 * per_sweep:3 * per_sweep]), '<f4').astype(np.float64)
    for j in range(k):                           # by the third sweep every capture is x
        assert relerr(10 ** (last[j * nbins:(j + 1) * nbins] / 10), 10 ** (ref_x / 10)) < RTOL


def test_spectrum_sweeper_sharded_stitcher_loop_world_1(ctx):
    """start_sharded: the rank-local stitcher loop over SweepPipeline (one rank here), captures already on the device."""
    import time
    import torch
    import ofdm_tools
    from ofdm_tools import packets
    rx = FakeReceiver()
    fft_len, Sf, tSf = 4096, 2000000, 1750000
    blk = ofdm_tools.spectrum_sweeper(rx, 'rtl', fft_len, Sf, tSf, 100e6, 107e6, 15, 0.0, 8, 0, 1472, ctx=ctx,
                                      threaded=False)
    pts, tune, excess = R.sweeper_geometry(fft_len, Sf, tSf, 100e6, 107e6, 8)
    dev = torch.device('cuda', 0)
    vectors = [R.synth_iq(pts, 2100 + i) for i in range(len(tune))]
    tv = [torch.from_numpy(v).to(dev) for v in vectors]
    frames = []
    blk.msg_connect('pdus', lambda m: frames.append(m[1]))
    blk.start_sharded(lambda i, f: tv[i], 0, 1, dev, sweeps=3)
    end = time.monotonic() + 20
    while blk.keep_running and time.monotonic() < end:
        time.sleep(0.005)
    blk.stop()
    assert blk.sweeps_done == 3 and rx.tuned == tune * 3
    ref = R.sweeper_stitch(vectors, fft_len, Sf, excess, 0.0)
    per_sweep = packets.sweeper_fragment_count(4 * len(ref), 1470)
    assert len(frames) == 3 * per_sweep                         # every sweep published, the last one at the end
    for s in range(3):
        got = np.frombuffer(packets.reassemble(frames[s * per_sweep:(s + 1) * per_sweep]), '<f4').astype(np.float64)
        assert relerr(10 ** (got / 10), 10 ** (ref / 10)) < RTOL


def test_coherence_estimator_feeds_detector(ctx, golden):
    import ofdm_tools
    g = golden('coherence_csd_4096.npz')
    N, Sf, tune = 4096, 2000000, 433000000
    est = ofdm_tools.coherence_estimator(N, Sf, block_len=65536, ctx=ctx)
    est.work([g['x'], g['y']], [])
    assert np.max(np.abs(est.cxy - np.fft.fftshift(g['expected_cxy']))) < RTOL
    # x and y share the tones and the noise -> coherent everywhere the delayed copy dominates
    calls = []
    det = ofdm_tools.coherence_detector(N, Sf, threshold=1.2, threshold_mtm=0.2, tune_freq=tune,
                                        subject_channels=[tune + 0.1234 * Sf, tune - 0.31 * Sf],
                                        valve_callback=calls.append)
    quiet = np.zeros(N, np.float32)
    det.work([est.cxy.reshape(1, N), quiet.reshape(1, N), quiet.reshape(1, N)], [])
    coh, outcome, valve = R.coherence_scanner(np.fft.fftshift(g['expected_cxy']), quiet, quiet,
                                              det.idx_subject_channels, 1.2, 0.2)
    assert det.get_subject_channels_outcome() == outcome and calls == valve
    assert np.allclose(det.subject_channels_coherence, coh, atol=2e-4)


def test_legacy_spectrum_sensor_request_response(ctx, tmp_path):
    import ofdm_tools
    Sf, N = 1000000, 1024
    for method in ('welch', 'fft'):
        os.makedirs(str(tmp_path / method))
        blk = ofdm_tools.spectrum_sensor(8192, sample_rate=Sf, fft_len=N, channel_space=50e3, search_bw=25e3,
                                         method=method, thr_leveler=5, tune_freq=0, alpha_avg=1, ctx=ctx,
                                         log=True, log_dir=str(tmp_path / method))
        out = []
        blk.msg_connect('PDU spect_msg', out.append)
        x = R.synth_iq(20000, 41)
        assert blk.work([x], []) == 8192                    # consumes at most block_length items
        blk.post('PDU from_cogeng', ({}, 'SC'))
        thr, plc, noise, cons = R.fast_spectrum_scan(x[:8192], 0, 50e3, 25e3, N, Sf, method, 5, 1e-11, 1)
        got = dict(out)
        assert np.isclose(got['thre'], thr, rtol=1e-4) and np.isclose(got['nois'], noise, rtol=1e-4)
        assert got['cons'] == cons and len(cons) > 0
        assert np.allclose(blk.get_power_level_ch(), plc, rtol=1e-4)
        blk.post('PDU from_cogeng', ({}, 'PAPR'))
        blk.post('PDU from_cogeng', ({}, 'bogus'))
        assert out[-2][0] == 'papr' and out[-1] == ('unkn', 'received unknown request')
        # the request log of spectrum_sensor.py:59-62,96-120
        rows = [ln.split(',', 3) for ln in open(blk.log_file.path).read().splitlines()]
        assert [r[2] for r in rows] == ['sample_rate', 'tune_freq[Hz]', 'threshold[dB]', 'noise[dB]',
                                        'spectrum_constraint[Hz]', 'tune_freq', 'papr', 'received unknown request']
        assert np.isclose(float(rows[2][3]), 10 * np.log10(thr + 1e-20), atol=1e-3) and rows[4][3] == str(cons)


def test_legacy_spectrum_sensor_async_scan(ctx):
    """async_scan=True: 'SC' only enqueues (oth_welch_exec_async); the three PDUs leave from work() once the PSD is on the
    host, equal to the blocking block's; a second request while one is pending answers the older one first; the helpers'
    plans are built once per shape and reused."""
    import ofdm_tools
    from ofdm_tools import ofdm_cr_tools
    Sf, N = 1000000, 1024
    x = R.synth_iq(3 * 8192, 43)
    for method in ('welch', 'fft'):
        kw = dict(sample_rate=Sf, fft_len=N, channel_space=50e3, search_bw=25e3, method=method, thr_leveler=5,
                  tune_freq=0, alpha_avg=0.5, ctx=ctx)
        ref, blk = ofdm_tools.spectrum_sensor(8192, **kw), ofdm_tools.spectrum_sensor(8192, async_scan=True, **kw)
        want, out = [], []
        ref.msg_connect('PDU spect_msg', want.append)
        blk.msg_connect('PDU spect_msg', out.append)
        for k in range(3):                                  # the noise estimate carries from scan to scan
            seg = x[k * 8192:(k + 1) * 8192]
            ref.work([seg], [])
            ref.post('PDU from_cogeng', ({}, 'SC'))
            blk.work([seg], [])
            n_before = len(out)
            blk.post('PDU from_cogeng', ({}, 'SC'))
            assert len(out) == n_before                     # nothing published by the handler itself
            if k == 1:
                blk.post('PDU from_cogeng', ({}, 'SC'))     # a second request: the pending one is answered first
                assert len(out) == n_before + 3
                ref.post('PDU from_cogeng', ({}, 'SC'))
            for _ in range(2000):                           # work() never waits: poll it like the scheduler would
                blk.work([seg], [])
                if blk._scan is None:
                    break
            assert blk._scan is None and blk.collect_scan()
        assert [f for f, _ in out] == [f for f, _ in want] == ['thre', 'nois', 'cons'] * 4
        for (f, a), (_, b) in zip(out, want):
            assert a == b, (method, f)                      # the same kernels on the same samples: identical
        assert np.array_equal(blk.get_power_level_ch(), ref.get_power_level_ch())
    made = len(ctx._plans)
    ofdm_cr_tools.fast_spectrum_scan(x[:8192], 0, 50e3, 25e3, N, Sf, 'welch', 5, 1e-11, 1, ctx=ctx)
    ofdm_cr_tools.fast_spectrum_scan(x[:8192], 0, 50e3, 25e3, N, Sf, 'fft', 5, 1e-11, 1, ctx=ctx)
    assert len(ctx._plans) == made >= 2                     # the two scans above built nothing new
    with pytest.raises(ValueError):
        ofdm_cr_tools.SpectrumScan(x[:8192], 0, 50e3, 25e3, N, Sf, 'bogus', 5, 1, ctx)


def test_ref_legacy_spectrum_sensor_session(ctx, golden, tmp_path):
    """f3 against the reference's OWN spectrum_sensor methods (spectrum_sensor.py:73-206, ref_legacy_sensor.npz): one
    scripted session - SC, PAPR, an unknown request, two logged setters, a second SC whose noise estimate carries
    over, a message that is not a PDU - must publish the same PDUs in the same order and write the same log rows
    (field names and order exact, lists exact, dB values to 1e-3: the reference computed in float64)."""
    import ofdm_tools
    g = golden('ref_legacy_sensor.npz')
    x = golden(str(g['input_from']))['x']
    Sf, N = int(g['sample_rate']), int(g['fft_len'])
    for method in ('welch', 'fft'):
        os.makedirs(str(tmp_path / method))
        blk = ofdm_tools.spectrum_sensor(int(g[method + '_block_length']), sample_rate=Sf, fft_len=N,
                                         channel_space=float(g['channel_space']), search_bw=float(g['search_bw']),
                                         method=method, thr_leveler=int(g['thr_leveler']), tune_freq=float(g['tune_freq']),
                                         alpha_avg=float(g['alpha_avg']), ctx=ctx, log=True, log_dir=str(tmp_path / method))
        out = []
        blk.msg_connect('PDU spect_msg', out.append)
        assert blk.work([x], []) == blk.block_length
        blk.post('PDU from_cogeng', ({}, 'SC'))
        blk.post('PDU from_cogeng', ({}, 'PAPR'))
        blk.post('PDU from_cogeng', ({}, 'bogus'))
        blk.set_tune_freq(float(g['tune_freq2']))
        blk.set_thr_leveler(int(g['thr_leveler2']))
        assert blk.work([x[int(g['second_offset']):]], []) == blk.block_length
        blk.post('PDU from_cogeng', ({}, 'SC'))
        blk.post('PDU from_cogeng', '')
        assert [m[0] for m in out] == list(g[method + '_metas'])
        assert np.allclose([out[0][1], out[5][1]], g[method + '_thre'], rtol=1e-4)
        assert np.allclose([out[1][1], out[6][1]], g[method + '_nois'], rtol=1e-4)
        for k, (pdu, tune) in enumerate(((out[2], float(g['tune_freq'])), (out[7], float(g['tune_freq2'])))):
            ax = R.frange(tune - Sf / 2, tune + Sf / 2, float(g['channel_space']))
            assert [1.0 if a in pdu[1] else 0.0 for a in ax] == list(g[method + '_cons%d' % k])
        assert np.isclose(out[3][1], float(g[method + '_papr']), atol=1e-4) and out[4][1] == str(g[method + '_unkn'])
        want = [ln.split(',', 3) for ln in bytes(g[method + '_log']).decode('ascii').splitlines()]
        got = [ln.split(',', 3) for ln in open(blk.log_file.path).read().splitlines()][1:]      # [0]: the ctor's header row
        assert [r[2] for r in got] == [r[2] for r in want] and all(r[0] == 'Time' and len(r[1]) == 6 for r in got)
        for a, b in zip(got, want):
            if a[2] in ('threshold[dB]', 'noise[dB]', 'papr'):
                assert abs(float(a[3]) - float(b[3])) < 1e-3, (a, b)
            else:
                assert a[3:] == b[3:], (a, b)


def test_helper_functions_match_oracle(ctx):
    from ofdm_tools import ofdm_cr_tools as T
    x = R.synth_iq(40000, 9)
    Sf, N = 2000000, 2048
    assert np.isclose(T.welch_power_estimate(x, N, Sf, ctx), R.welch_power_estimate(x, N, Sf), rtol=1e-5)
    ax, db = T.welch_plot_dB(x, Sf, 1e6, N, ctx)
    ax2, db2 = R.welch_plot_dB(x, Sf, 1e6, N)
    assert np.allclose(ax, ax2) and np.max(np.abs(np.array(db) - np.array(db2))) < 1e-3
    assert np.isclose(T.clc_power_freq(x[:2000], N, Sf, ctx), R.clc_power_freq(x[:2000], N, Sf), rtol=1e-5)
    assert np.isclose(T.clc_power_freq(x[:5000], N, Sf, ctx), R.clc_power_freq(x[:5000], N, Sf), rtol=1e-5)   # truncating fft
    Fr = float(Sf) / N
    bb = T.frange(-Sf // 2, Sf // 2, 100e3)
    for fn_t, fn_r in ((T.src_power_welch, R.src_power_welch), (T.src_power_fft, R.src_power_fft)):
        v = x if fn_t is T.src_power_welch else x[:1500]
        psd, axis, plc = fn_t(v, len(v), N, Fr, Sf, bb, 50e3 / Fr, ctx)
        psd2, axis2, plc2 = fn_r(v, len(v), N, Fr, Sf, bb, 50e3 / Fr)
        assert relerr(psd, psd2) < RTOL and np.allclose(plc, plc2, rtol=1e-4) and np.allclose(axis, axis2)


def test_ref_fft_plot_and_time_domain_power_on_the_gpu(ctx, golden):
    """The product helpers of the same names (HIP periodogram, device reduction) against the reference's own
    fft_plot_dB / fft_plot_lin / clc_power_time / td_power_estimate (ref_fft_plot.npz)."""
    from ofdm_tools import ofdm_cr_tools as T
    g = golden('ref_fft_plot.npz')
    x = golden(str(g['input_from']))['x']
    Sf, fc, nfft = int(g['Sf']), float(g['fc']), int(g['nfft'])
    for tag in ('exact', 'short', 'long'):
        lo, hi = g[tag + '_range']
        v = x[lo:hi]
        ax, lin = T.fft_plot_lin(v, Sf, fc, nfft, ctx)
        ax2, db = T.fft_plot_dB(v, Sf, fc, nfft, ctx)
        assert np.array_equal(ax, g[tag + '_axis']) and ax == ax2
        # a single rectangular periodogram: its deepest bins sit 1e-7 of the peak, so rows are judged by ulps of the peak
        from test_hip_parity import check_single_rows
        check_single_rows(np.asarray(lin)[None, :], g[tag + '_lin'][None, :])
        strong = g[tag + '_lin'] > 1e-4 * g[tag + '_lin'].max()
        assert np.max(np.abs(np.array(db) - g[tag + '_db'])[strong]) < 1e-3
        assert np.isclose(T.clc_power_time(v, ctx), float(g[tag + '_power_time']), rtol=1e-5)
        assert np.isclose(T.td_power_estimate(v, Sf, ctx), float(g[tag + '_td_power']), rtol=1e-5)
    assert T.logger is __import__('ofdm_tools.sensing_log', fromlist=['logger']).logger      # the reference's import path


def test_ref_src_power_fft_and_fft_scan_on_the_gpu(ctx, golden):
    """a14 through the product helpers (HIP periodogram + device channel sums) against the reference's own
    `src_power_fft` / `fast_spectrum_scan(method='fft')` output (ref_src_power_fft.npz)."""
    from ofdm_tools import ofdm_cr_tools as T
    g = golden('ref_src_power_fft.npz')
    x = golden(str(g['input_from']))['x']
    Sf, N = int(g['Sf']), int(g['nfft'])
    cs, sbw = float(g['channel_rate']), float(g['srch_bw'])
    Fr = float(Sf) / N
    bb = T.frange(-Sf // 2, Sf // 2, cs)
    psd, ax, plc = T.src_power_fft(x[:N], N, N, Fr, Sf, bb, sbw / Fr, ctx)
    assert relerr(psd, g['expected_psd']) < 1e-3 and np.allclose(ax, g['expected_axis'])      # single periodogram row ...
    amp = np.abs(np.sqrt(np.asarray(psd, np.float64)) - np.sqrt(g['expected_psd'])) / np.sqrt(g['expected_psd'].max())
    assert amp.max() <= 4 * 2.0 ** -23                                                         # ... held to 4 ulp of its peak
    assert np.allclose(plc, g['expected_plc'], rtol=1e-4)
    lo, hi = (int(v) for v in g['short_range'])
    psd, _, plc = T.src_power_fft(x[lo:hi], hi - lo, N, Fr, Sf, bb, sbw / Fr, ctx)
    assert np.allclose(plc, g['expected_plc_short'], rtol=1e-4)
    thr, plc, ne, occ = T.fast_spectrum_scan(x[:N], float(g['scan_fc']), cs, sbw, N, Sf, 'fft', int(g['scan_thr_leveler']),
                                             float(g['scan_noise0']), float(g['scan_alpha']), ctx=ctx)
    assert np.isclose(thr, float(g['scan_thr']), rtol=1e-4) and np.allclose(plc, g['scan_plc'], rtol=1e-4)
    ax_ch = T.frange(float(g['scan_fc']) - Sf // 2, float(g['scan_fc']) + Sf // 2, cs)
    assert [1.0 if a in occ else 0.0 for a in ax_ch] == list(g['scan_occupied'])


def test_batched_scan_config5(ctx):
    """64-channel-style batch (here 5 streams x 4 vectors of 16384): PSD rows, per-bin mask, channel powers."""
    from ofdm_tools.scan_batch import BatchScanPlan
    N, Sf, ns, n = 16384, 1000000, 5, 16384 * 4
    xs = [R.synth_iq(n, 3000 + i) for i in range(ns)]
    buf = np.concatenate(xs)
    plan = BatchScanPlan(ctx, N, Sf, 15625.0, 10e3, thr_leveler=3)
    d_in, d_out = ctx.alloc(buf.nbytes), ctx.alloc(ns * N * 4)
    try:
        ctx.h2d(d_in, buf)
        assert plan.psd_rows_dev(d_in, n, ns, n, d_out) == 4
        rows = ctx.d2h(d_out, (ns, N), np.float32)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    mask, noise, plc = plan.decide(rows)
    st = R.ScannerState(N, Sf, 15625.0, 10e3, trunc_band=Sf)
    for i, x in enumerate(xs):
        ref = R.chain_sensor_v2(x, N).mean(axis=0)
        assert relerr(rows[i], ref) < RTOL
        ma = R.movingaverage(ref, st.srch_bins)
        assert np.isclose(noise[i], ma.min(), rtol=1e-4)
        want = ref > 3 * ma.min()
        margin = np.abs(ref - 3 * ma.min()) > 1e-3 * ref          # bins that are not on the decision edge
        assert np.array_equal(mask[i].astype(bool)[margin], want[margin])
        assert 0 < mask[i].sum() < N                                # tones above, noise floor below
        assert np.allclose(plc[i], R.src_power(ref, N, st.Fr, Sf, st.bb_freqs, st.srch_bins), rtol=1e-4)


TORCH_STREAM_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/gr-ofdm_tools_amd')
import numpy as np, torch                      # torch first: both then share ONE HIP runtime (torch's)
from ofdm_tools import _hip, windows
from oracle import ref_cpu as R
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    c2 = _hip.Context(0, stream=s.cuda_stream)
    x = R.synth_iq(40000, 4)
    xt = torch.from_numpy(x.view(np.float32).copy()).cuda()
    out = torch.empty(4096, dtype=torch.float32, device='cuda')
    plan = c2.welch_plan(4096, window=windows.get_window('hann', 4096))
    assert plan.exec_dev(xt.data_ptr(), len(x), out.data_ptr()) == 18
    s.synchronize()
_, ref = R.welch_np(x, nperseg=4096, nfft=4096)
err = float(np.max(np.abs(out.cpu().numpy() - ref) / ref))
assert err < 1e-4, err
print('ok', err)
'''


def test_context_on_torch_stream(tmp_path):
    """oth_ctx_create_on_stream: the library runs on a caller-owned HIP stream (torch's).  Own process,
    torch imported first, as bench.py does - the library then binds to the HIP runtime torch loaded."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'torch_stream.py'
    script.write_text(TORCH_STREAM_SCRIPT % {'root': root})
    p = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()


def test_flanck_detector_edges(ctx, tmp_path):
    """A burst that switches on and off in one subject channel: one rising and one falling edge there,
    the same sequence as the oracle's restatement of flanck_detector.py:345-399."""
    import ofdm_tools
    N, Sf, cs = 1024, 1024000, 32000.0
    st0 = R.ScannerState(N, Sf, cs, 16e3, trunc_band=Sf)
    subj = [st0.ax_ch[10], st0.ax_ch[20]]
    f_on = (st0.ax_ch[20]) / Sf                                     # tone in the middle of channel 20
    nvec = 30
    x = R.synth_iq(N * nvec, 71, tones=(), dc=0)
    t = np.arange(N * nvec)
    gate = ((t // N >= 8) & (t // N < 18)).astype(np.float64)        # on for vectors 8..17
    x = (x + 3.0 * gate * np.exp(2j * np.pi * f_on * t)).astype(np.complex64)
    kw = dict(channel_space=cs, search_bw=16e3, thr_leveler=4, alpha_avg=0.2, trunc_band=Sf, peak_alpha=0.5)
    blk = ofdm_tools.flanck_detector(N, Sf / N, Sf, subject_channels=subj, ctx=ctx, threaded=False, log_directory=str(tmp_path), **kw)
    ref = R.FlankState(N, Sf, cs, 16e3, subj, trunc_band=Sf, thr_leveler=4, alpha_avg=0.2, peak_alpha=0.5)
    rows = R.chain_sensor_v2(x, N)
    want = []
    for i in range(nvec):
        blk.work([x[i * N:(i + 1) * N]], [])
        want += ref.detect(rows[i].astype(np.float32))
        assert np.allclose(blk.curr_power, ref.curr_power, rtol=1e-4) and blk.flag == ref.flag
    assert blk.events == want
    ch20 = [e for e in blk.events if e[0] == subj[1]]
    assert (subj[1], +1) in ch20 and ch20[-1] == (subj[1], -1)
    assert blk._logger.cumulative_statistics == ref.cumulative_statistics


def test_ref_flank_detector_through_the_block(ctx, golden, tmp_path):
    """f4 against the reference's OWN flank_detector (flanck_detector.py:345-399, ref_flank.npz): the committed IQ
    through the block, one vector per work() call - peak-tracking power, flags and edge counts row by row."""
    import ofdm_tools
    g = golden('ref_flank.npz')
    N, Sf = int(g['fft_len']), int(g['sample_rate'])
    subj = [float(c) for c in g['subject_channels']]
    blk = ofdm_tools.flanck_detector(N, Sf / N, Sf, subject_channels=subj, ctx=ctx, threaded=False,
                                     log_directory=str(tmp_path), channel_space=float(g['channel_space']),
                                     search_bw=float(g['search_bw']), thr_leveler=int(g['thr_leveler']),
                                     alpha_avg=float(g['alpha_avg']), trunc_band=Sf, peak_alpha=float(g['peak_alpha']))
    x = g['x']
    for i in range(len(g['rows'])):
        blk.work([x[i * N:(i + 1) * N]], [])
        assert np.allclose(blk.curr_power, g['curr_power_seq'][i], rtol=1e-4), i
        assert [1.0 if f else 0.0 for f in blk.flag] == list(g['flag_seq'][i]), i
    stats = blk._logger.cumulative_statistics
    assert sorted(stats) == list(g['stat_channels']) and [stats[k] for k in sorted(stats)] == list(g['stat_counts'])
    blk.stop()


def test_two_threads_share_one_context():
    """GNU Radio gives every block its own scheduler thread and the blocks of a process share the default
    context: two threads hammer one context with different plans (ctypes drops the GIL during the calls);
    every result must equal the single-threaded one."""
    import threading
    from ofdm_tools import _hip, windows
    ctx = _hip.Context(0)
    try:
        xa = R.synth_iq(4096 + 2048 * 400, 501)
        xb = R.synth_iq(2048 * 300, 502)
        pa = ctx.welch_plan(4096, window=windows.get_window('hann', 4096))
        pb = ctx.welch_plan(2048, window=windows.get_window('flattop', 2048), fs=2e6, fftshift=True)
        want_a, want_b = pa.exec(xa).copy(), pb.exec(xb).copy()
        errors = []

        def worker(plan, x, want):
            try:
                for _ in range(150):
                    got = plan.exec(x)
                    if float(np.max(np.abs(got - want) / want)) > 2e-5:
                        errors.append('mismatch')
                        return
            except Exception as e:      # noqa: BLE001 - report anything from the worker thread
                errors.append(repr(e))

        ts = [threading.Thread(target=worker, args=a) for a in ((pa, xa, want_a), (pb, xb, want_b))]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
        assert not errors, errors
    finally:
        ctx.close()


# ---- asynchronous work() and the lossy depth-2 transport (SURVEY.md 8a row a15, 8b contract row) --------------

def test_work_returns_before_the_gpu_is_done_and_results_match_the_sync_path(ctx):
    """oth_chain_push_async: work() enqueues (pinned copy, H2D, kernels, D2H of the latest row, event) and
    returns; poll() is non-blocking; the collected rows equal the synchronous oth_chain_push path."""
    from ofdm_tools import _hip, windows
    N = 2048
    x = R.synth_iq(N * 4096, 71)                       # 64 MiB per push: the copy alone takes > 1 ms
    k = -10 * np.log10(N) - 10 * np.log10(2.0e6)
    ref = ctx.chain(N, windows.blackmanharris(N), True, _hip.EPI_MAG2, 1)
    ref.set_iir_log(0.8, k)
    want = [ref.push(x, max_rows=1)[0][-1].copy() for _ in range(3)]
    ch = ctx.chain(N, windows.blackmanharris(N), True, _hip.EPI_MAG2, 1)
    ch.set_iir_log(0.8, k)
    tickets = [ch.push_async(x) for _ in range(3)]     # three pushes back to back: the GPU is busy for several ms
    assert ch.poll(tickets[-1]) is None                # the call returned before its event completed
    for t, w in zip(tickets, want):
        row, n = ch.wait(t)
        assert n == 4096 and relerr(10 ** (row / 10.0), 10 ** (w / 10.0)) < 1e-5
    assert ch.poll(tickets[-1]) is not None
    # the ring keeps four tickets: the oldest of six is gone (latest wins)
    more = [ch.push_async(x[:N * 8]) for _ in range(6)]
    with pytest.raises(_hip.HipError) as ei:
        ch.wait(more[0])
    assert ei.value.code == -5
    assert ch.wait(more[-1])[1] == 8


def test_threaded_watcher_drops_when_stalled_and_never_back_pressures(ctx, golden):
    """threaded=True: work() hands tickets to a depth-2 lossy queue; a stalled watcher loses vectors
    (LossyQueue.dropped > 0) while work() keeps returning at once; what the watcher does process equals the
    inline path's result for the same vector."""
    import threading
    import time
    import ofdm_tools
    g = golden('scanner_state_seq.npz')
    kw = dict(channel_space=25e3, search_bw=12.5e3, thr_leveler=4, tune_freq=100000000, alpha_avg=0.5,
              trunc_band=800000, stats=True, ctx=ctx)
    x = g['x']
    inline = ofdm_tools.spectrum_sensor_v2(1024, 1000, 1000000, threaded=False, **kw)
    inline.work([x[:1024]], [])
    blk = ofdm_tools.spectrum_sensor_v2(1024, 1000, 1000000, threaded=True, **kw)
    gate = threading.Event()
    seen = []
    real = blk._on_vector

    def slow(row):
        seen.append(row.copy())
        gate.wait(5.0)                                  # the watcher is stuck in its first vector
        real(row)
    blk._on_vector = slow
    t0 = time.perf_counter()
    for i in range(16):
        assert blk.work([x[i * 1024:(i + 1) * 1024]], []) == 1024
    dt = time.perf_counter() - t0
    assert dt < 1.0, dt                                 # sixteen calls, none waited for the stalled watcher
    # depth 2: the one in progress + two queued survive - and whatever the watcher had already taken off the queue while
    # it still waited for the FIRST row to come back from the GPU (a busy device: one or two more)
    assert blk.msgq0.dropped >= 10
    gate.set()
    deadline = time.time() + 5.0
    while blk.msgq0.count() and time.time() < deadline:
        time.sleep(0.01)
    time.sleep(0.1)
    blk.stop()
    assert 1 <= len(seen) <= 3 and len(seen) + blk.vectors_lost + blk.msgq0.dropped >= 16 - 2
    assert relerr(seen[0], R.chain_sensor_v2(x[:1024], 1024)[0]) < RTOL
    # the first processed vector gave the same scanner state as the inline block's
    assert blk._scanner.n_measurements == len(seen) - blk.vectors_lost or blk._scanner.n_measurements >= 1


def test_strobes_reemit_and_file_logger_thread(ctx, golden, tmp_path):
    """What start() adds (spectrum_sensor_v2.py:108-111,125-129; ofdm_cr_tools.py:1906,2010-2107): the top-4
    frequencies are re-emitted every strobe period, and the file_logger thread writes the logs periodically
    and once more when it stops."""
    import time
    import ofdm_tools
    g = golden('scanner_state_seq.npz')
    subj = list(g['subject_channels'])
    blk = ofdm_tools.spectrum_sensor_v2(1024, 1000, 1000000, channel_space=25e3, search_bw=12.5e3, thr_leveler=4,
                                        tune_freq=100000000, alpha_avg=0.5, trunc_band=800000, stats=True, psd=True,
                                        output='o', subject_channels=subj, ctx=ctx, threaded=False, log_directory=str(tmp_path),
                                        period=0.05, test_duration=0.2, strobe_period_ms=20)
    msgs = []
    blk.msg_connect('freq_out_0', msgs.append)
    blk.start()
    blk.feed(g['x'], max_items=1024)
    time.sleep(0.3)
    blk.stop()
    assert blk.top4 == list(g['top4'])
    assert len(msgs) >= 5 and msgs[-1][1] == g['top4'][0] - 100000000      # re-emitted, not only once
    assert blk._logger.files_written >= 3                                   # periodic passes + the last write
    import glob
    assert glob.glob(str(tmp_path / 'sdr_psd_cumulative_log-*.matz')) and \
        len(glob.glob(str(tmp_path / 'sdr_ss_periodic_log-*.log'))) >= 1


def test_waterfall_block_end_to_end(ctx, tmp_path):
    """waterfall=True (spectrum_sensor_v2.py:98-107,121-122,304-322): the PSD vector stream goes through
    keep_one_in_n(sens_per_sec) into the waterfall watcher, which appends the vector to the logger's
    cumulative_waterfall; file_logger appends the rows as '%1.2e' CSV (ofdm_cr_tools.py:2039-2046).  Rows must be the
    LAST vector of every group of sens_per_sec PSD vectors, whatever the work() chunking."""
    import glob
    import ofdm_tools
    N, S = 256, 5
    x = R.synth_iq(N * 23 + 40, 71)
    ref = R.chain_sensor_v2(x, N)                      # decimation 1: every vector is a PSD row
    want = ref[S - 1::S][:len(ref) // S]
    for chunk in (N, 3 * N + 17, 11 * N):              # one vector per work() call; calls that straddle vectors;
                                                       # calls that span two groups (one message -> ONE row, :308-313)
        blk = ofdm_tools.spectrum_sensor_v2(N, S, N * S, waterfall=True, ctx=ctx, threaded=False,
                                            log_directory=str(tmp_path / ('c%d' % chunk)))
        assert blk.decimation == 1
        blk.feed(x, max_items=chunk)
        rows = np.array(blk._logger.cumulative_waterfall)
        if chunk == N:                                 # exact: the group's last vector is the call's last vector
            from test_hip_parity import check_single_rows
            assert rows.shape == want.shape
            check_single_rows(rows, want)
        elif chunk == 11 * N:                          # 23 vectors in calls of 11, 11, 1: rows 10 and 21, nothing else
            assert len(rows) == 2
            check = __import__('test_hip_parity').check_single_rows
            check(rows, ref[[10, 21]])
        else:                                          # one row per completed group, each a PSD row at or after the group's last
            assert len(rows) == len(want)
            for i, r in enumerate(rows):
                j = next(j for j in range((i + 1) * S - 1, len(ref)) if relerr(r, ref[j]) < 1e-3)
                assert j - ((i + 1) * S - 1) < 4
        out = blk._logger.flush()
        txt = open(out['waterfall']).read().strip().split('\n')
        assert len(txt) == len(rows) and txt[0].split(',')[0] == '%1.2e' % rows[0][0]
        assert len(txt[0].split(',')) == N
        assert blk._logger.cumulative_waterfall == []          # a new period starts empty, the file keeps appending
        assert glob.glob(str(tmp_path / ('c%d' % chunk) / 'sdr_waterfall_cumulative_log-*.matz'))


def test_default_work_never_waits_for_the_gpu(ctx):
    """Every chain block runs its watcher thread by default, as the reference does (spectrum_sensor_v2.py:138-155):
    work() enqueues and returns; the vector's effects appear once the watcher has collected the ticket."""
    import inspect
    import time
    import ofdm_tools
    from ofdm_tools import chain_block
    for cls in (ofdm_tools.spectrum_sensor_v2, ofdm_tools.spectrum_sensor_v1, ofdm_tools.psd_logger,
                ofdm_tools.local_worker, ofdm_tools.multichannel_scanner, ofdm_tools.flanck_detector,
                ofdm_tools.ascii_plot):
        assert inspect.signature(cls.__init__).parameters['threaded'].default is True, cls
    seen = []
    blk = ofdm_tools.spectrum_sensor_v2(4096, 1000, 4096 * 1000, channel_space=25e3, search_bw=12.5e3, ctx=ctx)
    assert blk._threaded and blk._watch_thread.is_alive()
    inner = blk._on_vector
    blk._on_vector = lambda row: (seen.append(row.copy()), inner(row))
    x = R.synth_iq(4096 * 64, 5)
    done = ctx.chain(4096, None, True, 2, 1)           # an unrelated long launch queued first on the same stream
    d = ctx.alloc(8 << 26)
    try:
        ctx.synth_iq(d, 1 << 26, 3, R.TONES, R.DC)
        done.push_dev(d, 1 << 26)
        t0 = time.perf_counter()
        assert blk.work([x], []) == len(x)
        dt = time.perf_counter() - t0
        assert blk.drain(10.0)
    finally:
        ctx.free(d)
    blk.stop()
    assert len(seen) == 1 and relerr(seen[0], R.chain_sensor_v2(x, 4096)[-1]) < 1e-3
    assert dt < 0.05, dt                               # (the enqueue; the GPU work behind it is not waited for)
    assert chain_block.ChainBlockMixin._chain_init.__defaults__ == (True,)


def test_pinned_source_buffers_are_copied_before_the_call_returns(ctx):
    """A caller's buffer is only valid during work() (python/spectrum_sensor.py:71-75).  Pageable memory is staged by
    the runtime before hipMemcpyAsync returns; a PINNED / registered buffer (a torch pinned tensor, a registered
    scheduler buffer) would be read asynchronously - the library must have copied it when the call returns.  Scribble
    over the buffer right after push_async / accumulate and compare with the untouched run."""
    import torch
    n = 1 << 18                                        # 2 MiB: above the pinned-ring threshold of the large-copy path
    x = R.synth_iq(n, 91)
    pinned = torch.empty(n * 2, dtype=torch.float32).pin_memory()
    view = pinned.numpy().view(np.complex64)
    for _ in range(3):
        view[:] = x
        ch = ctx.chain(1024, None, True, 2, 1)
        t = ch.push_async(view)
        view[:] = 0                                    # the scheduler reuses its buffer
        row, k = ch.wait(t)
        assert k == n // 1024 and relerr(row, R.chain_sensor_v2(x[-1024:], 1024)[0]) < 1e-3
        ch.close()
        view[:] = x
        plan = ctx.welch_plan(1024, window=None)
        plan.accumulate(view)
        view[:] = 0
        psd = plan.finalize()
        want = ctx.welch_plan(1024, window=None).exec(x)
        assert relerr(psd, want) < 1e-5
        plan.close()
    # a pinned source past 64 MiB is not copied into the ring (that would pin as much again): its DMA is enqueued
    # directly and the call waits for that copy alone
    nbig = (72 << 20) // 8
    big = torch.empty(nbig * 2, dtype=torch.float32).pin_memory()
    bv = big.numpy().view(np.complex64)
    bv[:] = np.resize(x, nbig)
    plan = ctx.welch_plan(1024, window=None)
    plan.accumulate(bv)
    bv[:] = 0
    psd = plan.finalize()
    assert relerr(psd, ctx.welch_plan(1024, window=None).exec(np.resize(x, nbig))) < 1e-5
    ch = ctx.chain(4096, None, True, 2, 1)
    bv[:] = np.resize(x, nbig)
    t = ch.push_async(bv)
    bv[:] = 0
    row, k = ch.wait(t)
    assert k == nbig // 4096 and relerr(row, R.chain_sensor_v2(np.resize(x, nbig)[-4096 - nbig % 4096:][:4096], 4096)[0]) < 1e-3


# ---- multi-GPU host paths on one GPU (world 1 and ranks simulated one after another) -------------------------

def test_long_stream_welch_and_coherence_through_the_hip_plans(ctx, golden):
    """ofdm_tools.sweep.welch_long_stream / csd_long_stream on device buffers: with
    world = 1 they equal the one-shot plan; with three ranks run one after another (each given only its time run +
    halo, partials summed the way reduce_partials does) they equal it too."""
    import torch
    from ofdm_tools import sweep, windows
    g = golden('coherence_csd_4096.npz')
    dev = torch.device('cuda', 0)
    x = torch.from_numpy(g['x'].view(np.float32).reshape(-1, 2)).to(dev)
    y = torch.from_numpy(g['y'].view(np.float32).reshape(-1, 2)).to(dev)
    torch.cuda.synchronize()
    n = x.shape[0]
    plan = ctx.welch_plan(4096, window=windows.get_window('hann', 4096), fs=1.0)
    want = plan.exec(g['x'])
    psd, nseg = sweep.welch_long_stream(plan, x.data_ptr(), 0, n, dev, 0, 1)
    assert nseg == 31 and relerr(psd.cpu().numpy(), want) < 2e-6
    (pxx, pyy, pxy, cxy), nseg = sweep.csd_long_stream(plan, x.data_ptr(), y.data_ptr(), 0, n, dev, 0, 1)
    w = plan.csd(g['x'], g['y'])
    assert nseg == 31 and relerr(pxx.cpu().numpy(), w[0]) < 2e-6 and relerr(pyy.cpu().numpy(), w[1]) < 2e-6
    assert np.max(np.abs(cxy.cpu().numpy() - w[3])) < 1e-5
    assert np.max(np.abs(cxy.cpu().numpy() - g['expected_cxy'])) < RTOL
    # three ranks, one after another: each sees only its own chunk of the stream
    world, total, count = 3, torch.zeros(4096, dtype=torch.float64, device=dev), 0
    for r in range(world):
        first, cnt, s0, k = sweep.time_shard(n, 4096, 2048, r, world)
        local = x[first:first + cnt].contiguous()
        part = torch.zeros(4096, dtype=torch.float32, device=dev)
        sweep.torch_then_ctx(ctx, dev)       # `ctx` runs on its own stream: torch's copy and fill must have landed
        assert plan.partial_dev(local.data_ptr(), cnt, part.data_ptr()) == k
        sweep.ctx_then_torch(ctx)
        total += part.to(torch.float64)
        count += k
    out = torch.empty(4096, dtype=torch.float32, device=dev)
    sums = total.to(torch.float32)
    sweep.torch_then_ctx(ctx, dev)
    plan.scale_dev(sums.data_ptr(), count, out.data_ptr())
    sweep.ctx_then_torch(ctx)
    assert count == 31 and relerr(out.cpu().numpy(), want) < 2e-6


def test_batched_scanner_sharded_entry_point_world_1(ctx):
    """BatchScanPlan.scan_sharded with one rank: rows, noise floors and channel powers in
    channel order equal the unsharded device path."""
    import torch
    from ofdm_tools.scan_batch import BatchScanPlan
    N, nch, n = 16384, 3, 16384 * 4
    dev = torch.device('cuda', 0)
    bp = BatchScanPlan(ctx, N, 1000000, 15625.0, 10e3, thr_leveler=3.0)
    iq = torch.empty((nch * n, 2), dtype=torch.float32, device=dev)
    ctx.synth_iq(iq.data_ptr(), nch * n, 3000, R.TONES, R.DC)
    ctx.sync()
    rows, noise, power = bp.scan_sharded(iq.data_ptr(), n, n, nch, 0, 1, dev)
    d_rows = ctx.alloc(nch * N * 4)
    try:
        bp.psd_rows_dev(iq.data_ptr(), n, nch, n, d_rows)
        mask, noise2, plc = bp.decide_dev(d_rows, nch)
        want_rows = ctx.d2h(d_rows, (nch, N), np.float32)
    finally:
        ctx.free(d_rows)
    assert np.array_equal(rows.cpu().numpy(), want_rows)
    assert np.allclose(noise.cpu().numpy(), noise2) and np.allclose(power.cpu().numpy(), plc)


def test_ascii_plot_block(ctx):
    """ascii_plot (python/ascii_plot.py): rectangular shifted FFT -> |.|^2 -> IIR -> log chain on the GPU, latest
    row rendered by make_plot and posted on pkt_out; against the oracle's chain + renderer."""
    import ofdm_tools
    N, Sf = 1024, 1024 * 30
    blk = ofdm_tools.ascii_plot(N, Sf, 433.0e6, 0.3, 10, 64, 20, ctx=ctx, threaded=False)
    assert blk._decimation() == 3
    msgs = []
    blk.msg_connect('pkt_out', msgs.append)
    x = R.synth_iq(N * 31 + 5, 77)
    blk.feed(x, max_items=4000)
    lin, db = R.chain_ascii_plot(x, N, Sf, 0.3, decim=3)
    assert len(db) == 10
    assert relerr(blk._chain.iir(), lin[-1]) < RTOL
    want = R.ascii_make_plot(db[-1].astype(np.float32), 64, 20, 433.0e6, Sf, N)
    assert msgs and msgs[-1][1] == blk.last_plot
    # the picture is a quantisation of the dB row: identical up to bars that sit within rounding of a row boundary
    got_rows, want_rows = blk.last_plot.split('\n'), want.split('\n')
    assert len(got_rows) == len(want_rows) and got_rows[-2:] == want_rows[-2:]
    diff = sum(a != b for a, b in zip(blk.last_plot, want))
    assert diff <= 8, diff


def test_bench_gpus_2_spawns_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` as typed (no launcher): the parent spawns two ranks before it touches the GPU, rank 0's
    ONE JSON line comes back, rc 0.  Rehearsal form on this one-GPU box (both ranks on device 0, gloo)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env['BENCH_REHEARSE'] = '1'
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '5', '--warmup', '2',
                        '--sweep-log2-samples', '22', '--ramp-ms', '20', '--full'], env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r['n_gpus'] == 2 and r['steps'] == 5 and r['scaling'] == 'strong' and r['value'] > 0
    assert r['ranks_seen']['world_size'] == 2 and len(r['ranks_seen']['devices']) == 2
    assert 'sweep_c4.value' in r['scaling_base'] and r['parity_prefix_max_rel_err'] < RTOL


def test_full_size_config4_sweep_properties(ctx):
    """BASELINE config 4 at its own shape - 8 RF segments of 2^25 samples each (2 GiB on the device; the oracle cannot run
    there) - through the block's sharded sweep (spectrum_sweeper.sweep_once_sharded, the reference's own call: flattop,
    nperseg = 1024 zero-padded to 4096, spectrum_sweeper.py:260-276) and through the pipelined form bench.py times
    (sweep.SweepPipeline, Hann nperseg = 4096), at world 1:
      (1) the stitched PSD is the eight per-segment rows in TUNE order (every segment has its own seed and its own tone);
      (2) tuned against the independent coverage kernel on every segment, both calls (2e-5);
      (3) Parseval per segment: sum_k P[k] fs / nfft = the segment's sample variance (2e-3: a Welch estimate);
      (4) the 2^20-sample prefix of every segment against the float64 oracle (1e-4), both calls;
      (5) the pipeline's second sweep on the other buffer set equals its first."""
    import torch
    import ofdm_tools
    from ofdm_tools import _hip, sweep, windows
    nseg_rf, S, N, Sf, tSf, trim = 8, 1 << 25, 4096, 2000000, 1750000, 256
    dev = torch.device('cuda', 0)
    rx = FakeReceiver()
    blk = ofdm_tools.spectrum_sweeper(rx, 'rtl', N, Sf, tSf, 100e6, 100e6 + tSf * nseg_rf - 1, 15, 0.0, 8, 0, 1472, ctx=ctx,
                                      threaded=False)
    assert len(blk.tune_frequencies) == nseg_rf and blk.excess_bins == trim
    nb = N - 2 * trim
    seg = []
    for i in range(nseg_rf):                                   # segment i: seed 2000 + i and a marker tone of its own
        t = torch.empty((S, 2), dtype=torch.float32, device=dev)
        ctx.synth_iq(t.data_ptr(), S, 2000 + i, ((0.5, 0.1234), (2.0, -0.35 + 0.1 * i)), 0.1 + 0.05j)
        seg.append(t)
    torch.cuda.synchronize()
    asked = []

    def capture(i, f):
        asked.append((i, f))
        return seg[i]
    wide = blk.sweep_once_sharded(capture, 0, 1, dev)
    assert asked == list(enumerate(blk.tune_frequencies))
    assert wide.shape == (nseg_rf * nb,) and np.all(np.isfinite(wide))
    rows = 10 ** (wide.reshape(nseg_rf, nb) / 10)
    fl = windows.get_window('flattop', N // 4)
    hn = windows.get_window('hann', N)
    calls = {'ref': dict(nperseg=N // 4, window=fl), 'hann': dict(window=hn)}
    out = torch.empty(nb, dtype=torch.float32, device=dev)
    full = torch.empty(N, dtype=torch.float32, device=dev)
    pipe_rows = None
    for name, kw in calls.items():
        tuned = ctx.welch_plan(N, fs=float(Sf), fftshift=True, trim_bins=trim, db=True, kernel=_hip.KERNEL_TUNED, **kw)
        gen = ctx.welch_plan(N, fs=float(Sf), fftshift=True, trim_bins=trim, db=True, kernel=_hip.KERNEL_GENERIC, **kw)
        whole = ctx.welch_plan(N, fs=float(Sf), **kw)                      # untrimmed, linear: Parseval
        if name == 'hann':                                                  # (5) the pipelined form, two sweeps
            pipe = sweep.SweepPipeline(nseg_rf, nb, dev, 0, 1)

            def compute(i, out_row):
                sweep.torch_then_ctx(ctx, dev)
                tuned.exec_dev(seg[i].data_ptr(), S, out_row.data_ptr())
                sweep.ctx_then_torch(ctx)
            a = pipe.wideband(pipe.run(compute)).cpu().numpy().reshape(nseg_rf, nb)
            b = pipe.wideband(pipe.run(compute)).cpu().numpy().reshape(nseg_rf, nb)
            pipe.drain()
            assert relerr(10 ** (b / 10.0), 10 ** (a / 10.0)) < 2e-5      # (dynamic schedule: last bits may differ)
            pipe_rows = 10 ** (a.astype(np.float64) / 10)
        for i in range(nseg_rf):
            sweep.torch_then_ctx(ctx, dev)
            gen.exec_dev(seg[i].data_ptr(), S, out.data_ptr())
            whole.exec_dev(seg[i].data_ptr(), S, full.data_ptr())
            sweep.ctx_then_torch(ctx)
            g = 10 ** (out.cpu().numpy().astype(np.float64) / 10)
            mine = rows[i] if name == 'ref' else pipe_rows[i]
            assert relerr(mine, g) < 2e-5, (name, i, relerr(mine, g))                         # (1) + (2)
            # the segment's own marker tone sits where its seed says (tune order, not launch order)
            f0 = -0.35 + 0.1 * i
            kc = int(round(f0 * N)) % N
            ks = ((kc + N // 2) % N) - trim
            assert abs(int(np.argmax(mine)) - ks) <= 1, (name, i)
            mean, var = ctx.iq_power(seg[i].data_ptr(), S)
            p = full.cpu().numpy().astype(np.float64)
            assert abs(p.sum() * Sf / N - var) / var < 2e-3, (name, i)                         # (3)
            pre = seg[i][:1 << 20].cpu().numpy().view(np.complex64).reshape(-1)                # (4)
            if name == 'ref':
                want = 10 ** (R.sweeper_src_power(pre, N, float(Sf), trim) / 10)
            else:
                _, w = R.welch_np(pre, fs=float(Sf), nperseg=N, nfft=N)
                want = np.fft.fftshift(w)[trim:-trim]
            assert relerr(10 ** (tuned.exec(pre).astype(np.float64) / 10), want) < RTOL, (name, i)
        for pl in (tuned, gen, whole):
            pl.close()
    del seg
    torch.cuda.empty_cache()


def test_bench_gpus_4_rehearsal_two_segments_per_rank(tmp_path):
    """The N > 1 bench at world 4 on this one-GPU box (BENCH_REHEARSE=1: every rank on device 0 over gloo; the box allows
    six GPU processes, this test process is one of them, so the 8-rank spawn itself cannot be rehearsed here - the
    8-rank partition runs over gloo on the CPU, tests/test_host_logic_cpu.py): four children, two RF segments each (the
    G = 4 column of SURVEY 8e), tune order after the all-gather, ranks_seen, rank 0's single line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env['BENCH_REHEARSE'] = '1'
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '4', '--steps', '4', '--warmup', '1',
                        '--sweep-log2-samples', '20', '--ramp-ms', '10', '--full'], env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r['n_gpus'] == 4 and r['steps'] == 4 and r['scaling'] == 'strong' and r['value'] > 0
    assert r['ranks_seen']['world_size'] == 4 and len(r['ranks_seen']['devices']) == 4
    assert r['ranks_seen']['distinct_devices'] == 1 and r['ranks_seen']['backend'] == 'gloo'
    assert 'parallelism' in r['config'] and r['config']['parallelism'] == 'segment-per-gpu x4'
    assert r['parity_prefix_max_rel_err'] < RTOL and 'kernel=welch4096:ws' in r['roofline']['kernel']


@pytest.mark.parametrize('workload,ranks', [('c5', 2), ('c5', 4), ('c2', 2), ('c2', 4)])
def test_bench_workloads_c5_and_c2_over_ranks_rehearsal(workload, ranks):
    """Round 6: `bench.py --gpus N --workload c5 | c2` - the batched scanner (multichannel_scanner.py:78-100:
    64 channel rows over the ranks through BatchScanPlan.scan_sharded) and the long stream (row 2: sweep.welch_long_stream over
    time_shard) - rehearsed at 2 and 4 ranks on this one-GPU box (every rank on device 0, gloo), as the C4 sweep is."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env['BENCH_REHEARSE'] = '1'
    size = ['--scan-log2-samples', '18'] if workload == 'c5' else ['--log2-samples', '23']
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(ranks), '--workload', workload, '--steps', '4',
                        '--warmup', '1', '--ramp-ms', '10', '--full'] + size, env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r['n_gpus'] == ranks and r['steps'] == 4 and r['scaling'] == 'strong' and r['value'] > 0
    assert r['ranks_seen']['world_size'] == ranks and r['ranks_seen']['backend'] == 'gloo'
    assert r['parity_prefix_max_rel_err'] < RTOL
    if workload == 'c5':
        assert r['config']['parallelism'] == 'channel-stream-per-gpu x%d' % ranks and 'scan_c5.value' in r['scaling_base']
        assert 'welch16k1x' in r['roofline']['kernel']
    else:
        assert r['config']['parallelism'] == 'time-shard-per-gpu x%d' % ranks and '--gpus 1' in r['scaling_base']
        assert 'kernel=welch4096:ws' in r['roofline']['kernel']


def test_bench_plain_run_dumps_the_timed_psd(ctx, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the headline line only (no sub-objects, no CPU baseline, no
    parity), `steps` = K, and --dump-outputs writes the PSD of the last timed step - checked here against the oracle on the
    same seeded device input."""
    import json
    import subprocess
    import sys
    import torch
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    log2 = 22
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--ramp-ms', '10', '--log2-samples', str(log2), '--dump-outputs', str(tmp_path / 'out')],
                       env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r['steps'] == 3 and r['ms_per_step'] > 0 and r['value'] > 0 and r['unit'] == 'Msamples/s'
    assert r['higher_is_better'] is True and r['dtype'] == 'f32' and r['cpu_baseline'] is None
    assert not {'sweep_c4', 'csd_c3', 'scan_c5', 'host_visible_ms_per_step', 'parity_prefix_max_rel_err'} & set(r)
    assert sorted(os.listdir(str(tmp_path / 'out'))) == ['psd.npy']
    psd = np.load(str(tmp_path / 'out' / 'psd.npy'))
    assert psd.dtype == np.float32 and psd.shape == (bench.NFFT,)
    n = 1 << log2
    iq = torch.empty((n, 2), dtype=torch.float32, device='cuda:0')
    ctx.synth_iq(iq.data_ptr(), n, 1002, bench.TONES, bench.DC)
    ctx.sync()
    x = iq.cpu().numpy().view(np.complex64).reshape(-1)
    _, ref = R.welch_np(x, fs=1.0, nperseg=bench.NFFT, nfft=bench.NFFT)
    assert relerr(psd, ref) < RTOL


def test_full_size_config1_sensor_v2(ctx):
    """BASELINE config 1 at its OWN size (examples/spectrum_sensor_test.grc: samp_rate 1e6, channel spacing
    25 kHz, search bandwidth 12.5 kHz): 2^20 complex64 samples, fft_len 1024, rectangular |fftshift(FFT)|^2 / N^2,
    decimation 1 -> 1024 PSD rows, the 128 eight-row means, and per mean row the a7 channel sums + the a8 state machine
    (spectrum_sensor_v2.py:85-93,445-479).  Twice:
      * through the chain as the bench runs it - 8192-item pushes, every row kept: single rows by the 4-ulp criterion, the
        128 means (oth_rows_group_mean), channel sums (oth_channel_power) and the whole a8 state sequence against the
        oracle by the plain 1e-4;
      * through spectrum_sensor_v2.work() in 8192-item calls, as a GNU Radio scheduler would deliver them: the watcher sees
        the LAST vector of each call (message_sink(dont_block) + msg_queue(2), latest wins: a15), i.e. rows 7, 15, ... -
        128 scans, state against the oracle fed with exactly those rows."""
    import ofdm_tools
    from ofdm_tools import _hip, scanner
    from test_hip_parity import check_single_rows
    n, N, Sf, cs, sbw = 1 << 20, 1024, 1000000, 25e3, 12.5e3
    x = R.synth_iq(n, 1001)
    ref_rows = R.chain_sensor_v2(x, N)                      # [1024][1024] float64
    assert ref_rows.shape == (1024, N)
    ref_mean = ref_rows.reshape(128, 8, N).mean(axis=1)
    # -- the chain, every row
    ch = ctx.chain(N, None, True, _hip.EPI_MAG2_OVER_N2, 1)
    got = []
    for pos in range(0, n, 8192):
        rows, k = ch.push(x[pos:pos + 8192])
        assert k == 8
        got.append(rows.copy())
    rows = np.concatenate(got)
    assert rows.shape == (1024, N)
    check_single_rows(rows, ref_rows)
    mean8 = ctx.rows_group_mean(rows, 8)
    assert mean8.shape == (128, N) and relerr(mean8, ref_mean) < RTOL
    # the same 128 means in ONE launch, as bench.py's `c1` object forms them: each run of 8 vectors is a stream of a Welch plan
    # without overlap (rectangular, |X|^2 / N^2, shifted) - the batched scanner's form (scan_batch.BatchScanPlan)
    bp = ctx.welch_plan(N, noverlap=0, window=None, detrend=_hip.DETREND_NONE, scaling=_hip.SCALE_OVER_N2, fftshift=True)
    d_x, d_rows = ctx.alloc(n * 8), ctx.alloc(128 * N * 4)
    try:
        ctx.h2d(d_x, x)
        assert bp.exec_dev(d_x, 8192, d_rows, nstreams=128, stream_stride=8192) == 8
        assert relerr(ctx.d2h(d_rows, (128, N), np.float32), ref_mean) < RTOL
    finally:
        ctx.free(d_x)
        ctx.free(d_rows)
    sc = scanner.ChannelScanner(N, Sf, cs, sbw, trunc_band=Sf, thr_leveler=10, alpha_avg=0.5, ctx=ctx)
    st = R.ScannerState(N, Sf, cs, sbw, trunc_band=Sf, thr_leveler=10, alpha_avg=0.5)
    assert len(sc.ax_ch) == len(st.ax_ch) == 40
    for i in range(128):
        occ = sc.scan(mean8[i])
        _, occ_ref = st.scan(ref_mean[i].astype(np.float32))
        assert np.allclose(sc.plc, st.plc, rtol=1e-4) and np.isclose(sc.noise_estimate, st.noise_estimate, rtol=1e-4)
        assert occ == occ_ref, i
    assert np.allclose(sc.cumulative_max_power, st.cumulative_max_power, rtol=1e-4) and sc.n_measurements == 128
    # -- the block, 8192-item work() calls
    blk = ofdm_tools.spectrum_sensor_v2(N, 1000, Sf, channel_space=cs, search_bw=sbw, thr_leveler=10, alpha_avg=0.5,
                                        trunc_band=Sf, stats=True, ctx=ctx, threaded=False)
    assert blk.decimation == 1
    st = R.ScannerState(N, Sf, cs, sbw, trunc_band=Sf, thr_leveler=10, alpha_avg=0.5)
    for c in range(128):
        assert blk.work([x[c * 8192:(c + 1) * 8192]], []) == 8192
        st.scan(ref_rows[8 * c + 7].astype(np.float32))
        assert np.allclose(blk.power_level_ch, st.plc, rtol=1e-4) and np.isclose(blk.noise_estimate, st.noise_estimate, rtol=1e-4)
    assert blk._scanner.n_measurements == 128


def test_work_sized_pushes_cost_at_most_three_stream_operations(ctx):
    """Round 6 (verdict item 5): a GNU Radio scheduler hands work() 4 Ki - 32 Ki items (python/spectrum_sensor.py:71-75,
    spectrum_sensor_v2.py:85-97).  A steady-state push of that size enqueues at most THREE stream operations - the H2D copy,
    the transform kernel and, for the chains with IIR / peak-hold state, one state kernel; the latest row is written by the
    closing kernel straight into pinned host memory (no D2H copy behind it) - a push all of whose vectors keep_one_in_n
    drops enqueues NOTHING (no copy, no launch: spectrum_sensor_v2.py:86-87 keeps one vector in int(Sf / N / sens_per_sec)),
    and the host time of work() at 8192 items stays under 25 us (median).  Results: unchanged against the oracle."""
    import time
    import ofdm_tools
    N, Sf = 1024, 1024 * 1000
    x = R.synth_iq(8192 * 40, 91)
    mk = {
        'spectrum_sensor_v2': lambda: ofdm_tools.spectrum_sensor_v2(N, 1000, Sf, channel_space=Sf / 40.0, search_bw=Sf / 80.0,
                                                                     trunc_band=Sf, stats=True, ctx=ctx, threaded=False),
        'psd_logger': lambda: ofdm_tools.psd_logger(N, 1000, Sf, ctx=ctx, threaded=False, mat_file=os.devnull),
        'local_worker': lambda: ofdm_tools.local_worker(N, Sf, 0.3, 1000, 1472, True, ctx=ctx, threaded=False),
    }
    for name, make in mk.items():
        blk = make()
        seen = []
        blk._on_vector = seen.append
        host, ops = [], []
        for c in range(40):
            t0 = time.perf_counter()
            assert blk.work([x[c * 8192:(c + 1) * 8192]], []) == 8192
            host.append((time.perf_counter() - t0) * 1e6)
            ops.append(blk._chain.last_push_ops())
        assert max(ops[2:]) <= 3, (name, ops)
        assert len(seen) == 40
        blk.stop()
        # host time of the enqueue alone (threaded=False above waits for the row inside work(): measure push_async itself)
        ch = blk._chain
        t = []
        for c in range(40):
            t0 = time.perf_counter()
            ch.push_async(x[c * 8192:(c + 1) * 8192])
            t.append((time.perf_counter() - t0) * 1e6)
            if c % 3 == 2:
                ctx.sync()
        t.sort()
        print('%s: ops per 8192-item push %s, push_async median %.1f us' % (name, sorted(set(ops[2:])), t[len(t) // 2]))
        assert t[len(t) // 2] <= 25.0, (name, t[len(t) // 2])
    # results of the row-in-pinned-memory form against the oracle: rows 7, 15, ... of the rectangular chain; the IIR + log rows
    blk = mk['spectrum_sensor_v2']()
    rows = []
    blk._on_vector = lambda r: rows.append(r.copy())
    for c in range(40):
        blk.work([x[c * 8192:(c + 1) * 8192]], [])
    ref = R.chain_sensor_v2(x, N)[7::8]
    from test_hip_parity import check_single_rows
    check_single_rows(np.array(rows), ref)
    # keep_one_in_n drops everything in most pushes: decimation 100, 8 vectors per push -> 0 operations, ticket ready at once
    blk = ofdm_tools.spectrum_sensor_v2(N, 10, Sf, channel_space=Sf / 40.0, search_bw=Sf / 80.0, trunc_band=Sf, stats=True, ctx=ctx,
                                        threaded=False)
    assert blk.decimation == 100
    rows, ops = [], []
    blk._on_vector = lambda r: rows.append(r.copy())
    rng = np.random.default_rng(8)
    pos = 0
    while pos < len(x):
        m = int(rng.integers(1, 9000))
        blk.work([x[pos:pos + m]], [])
        ops.append(blk._chain.last_push_ops())
        pos += m
    ref = R.chain_sensor_v2(x, N, decim=100)
    assert len(rows) == len(ref) == 3
    check_single_rows(np.array(rows), ref)
    assert ops.count(0) >= len(ops) - 3 * 3, (len(ops), ops.count(0))      # only the pushes that touch a kept vector do anything
    # set_keep_one_in_n in mid-stream, row by row against GNU Radio's keep_one_in_n::set_n (d_n = d_count = n in front of
    # the vector still incomplete at the call; tests/test_chain_async_gpu.py has the other push forms and cases)
    ch = ctx.chain(N, None, True, _hip_epi(), 7)
    schedule = [(4900, 2)]
    ref = R.chain_sensor_v2(x[:20 * N], N, 7, schedule)
    kept = R.gr_kept_indices(20, N, 7, schedule)
    got, want = [], []
    for pos in range(0, 20 * N, 700):
        if pos == 4900:
            ch.set_keep_one_in_n(2)
        end = min(pos + 700, 20 * N)
        t = ch.push_async(x[pos:end])
        done = [i for i, v in enumerate(kept) if pos < (v + 1) * N <= end]      # (700 < N: one vector at most)
        assert ch.ticket_rows(t) == len(done), pos
        row, k = ch.wait(t)
        assert k == len(done), pos
        if k:
            got.append(row.copy())
            want.append(ref[done[-1]])
    ch.close()
    assert len(got) == len(kept) == 8
    check_single_rows(np.array(got), np.array(want))


def _hip_epi():
    from ofdm_tools import _hip
    return _hip.EPI_MAG2_OVER_N2
