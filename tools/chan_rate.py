#!/usr/bin/env python3
"""The polyphase channelizer's launch (oth_channelizer_push_dev: csrc/chanpfb.hip) on an MI355X: one push of 2^26
device-resident samples at (nchan, decim, taps) = (1024, 512, 8) and (4096, 4096, 4), timed with the context's timing events
(the launch alone, as bench.py times the headline), in Msamples/s and as a fraction of 8 TB/s at the algorithmic traffic of
8 (1 + nchan / decim) bytes per sample - every sample read once, nchan / decim outputs written per sample.

Next to it, in the same session and alternating: oth_welch_pfb_dev on the same samples, prototype and hop - the same fold
and transform with one row of sums in place of the output rows, so the difference is what the store costs.

No gate: the figures are the result.  -> profiles/chan_rate.txt

For the write counters run one shape alone under the profiler, counters only:
    rocprofv3 --pmc WRITE_SIZE -d DIR -- python tools/chan_rate.py 1 --only 1024 --out /dev/null
    rocprofv3 --pmc FETCH_SIZE -d DIR -- python tools/chan_rate.py 1 --only 1024 --out /dev/null
(FETCH_SIZE reads half of a wide coalesced read on gfx950.)

usage: chan_rate.py [reps] [--only NCHAN] [--out FILE]
"""
import sys

import numpy as np
import torch

from stat_time import Session

from ofdm_tools import windows  # noqa: E402 - stat_time sets the path

HBM_PEAK_GBPS = 8000.0
N = 1 << 26

only = None
if '--only' in sys.argv:
    i = sys.argv.index('--only')
    only = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
s = Session('chan_rate.txt', reps=10)
ctx, dev, say, reps = s.ctx, s.dev, s.say, s.reps


def kernel_ms(fn):
    """the launches of one call between the context's timing events -> (ms, launches)"""
    ctx.sync()
    ctx.set_timing(True)
    ctx.get_timing()
    fn()
    ctx.sync()
    ms, launches = ctx.get_timing()
    ctx.set_timing(False)
    return ms, launches


say('%s, one push of 2^26 samples, %d repetitions, the arms alternating' % (s.library, reps))
x = s.capture(N, dc=0j)
for nchan, decim, taps in ((1024, 512, 8), (4096, 4096, 4)):
    if only not in (None, nchan):
        continue
    h = windows.pfb_prototype(nchan, taps).astype(np.float32)
    chan = ctx.channelizer(nchan, decim, taps, h)
    frames = chan.frames_for(N)
    rows = torch.empty(2 * nchan * frames, dtype=torch.float32, device=dev)
    bank = ctx.welch_plan(nchan, noverlap=nchan - decim, window=windows.get_window('hann', nchan))
    bank.set_prototype(h, taps)
    row = torch.empty(nchan, dtype=torch.float32, device=dev)

    def run_chan():
        chan.reset()
        assert chan.push_dev(x.data_ptr(), N, rows.data_ptr(), frames) == frames

    def run_bank():
        assert bank.pfb_dev(x.data_ptr(), N, 1, N, row.data_ptr()) == frames

    for fn in (run_chan, run_bank, run_chan, run_bank):      # warm-up: workspaces, first launches
        fn()
    t_chan, t_bank = [], []
    for _ in range(reps):
        t_chan.append(kernel_ms(run_chan))
        t_bank.append(kernel_ms(run_bank))
    ms_chan, ms_bank = float(np.median([t[0] for t in t_chan])), float(np.median([t[0] for t in t_bank]))
    alg = 8.0 * (1.0 + float(nchan) / decim)      # bytes per sample
    say('')
    say('%d channels, hop %d, %d taps per branch: %d frames, %.0f MiB in, %.0f MiB out' %
        (nchan, decim, taps, frames, 8.0 * N / 2 ** 20, 8.0 * nchan * frames / 2 ** 20))
    say('  push_dev   %8.3f ms (median of %d, min %.3f; %d launch)  %8.0f Msamples/s  %.1f %% of 8 TB/s at %.0f bytes per sample   [%s]' %
        (ms_chan, reps, min(t[0] for t in t_chan), t_chan[0][1], N / ms_chan / 1e3, 100.0 * alg * N / (ms_chan * 1e-3) / 1e9 / HBM_PEAK_GBPS,
         alg, chan.last_recipe()))
    say('  pfb_dev    %8.3f ms (median of %d, min %.3f; %d launches) %8.0f Msamples/s  %.1f %% of 8 TB/s at 8 bytes per sample   [%s]' %
        (ms_bank, reps, min(t[0] for t in t_bank), t_bank[0][1], N / ms_bank / 1e3, 100.0 * 8.0 * N / (ms_bank * 1e-3) / 1e9 / HBM_PEAK_GBPS,
         bank.last_recipe()))
    say('  the output rows cost %.3f ms: push_dev / pfb_dev x%.2f; they leave at %.0f GB/s if all of the difference is theirs' %
        (ms_chan - ms_bank, ms_chan / ms_bank, 8.0 * nchan * frames / max(ms_chan - ms_bank, 1e-9) / 1e6))
    chan.close()
    bank.close()
    del rows, row
s.finish('kernel <N, T, F>', ('chan_pfb_kernel<',), key=lambda name, length: (length, name))
