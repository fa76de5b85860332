#!/usr/bin/env python3
"""Accuracy of one-segment 4096-point Hann rows through the forced role-split route (welch4096ws, tuning word 'ws')
against the float64 oracle, 12 seeds x 3 detrend modes: worst amplitude error in ulp of the row's peak amplitude and mean
relative power error, the figures of tools/archive/acc_probe.py for this kernel (profiles/ab_headline_symtw.txt).
usage: welch_row_probe.py   (OFDM_TOOLS_HIP_LIB selects another build)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gr-ofdm_tools_amd'))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from ofdm_tools import _hip, windows  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402

ctx = _hip.Context(0)
w = windows.get_window('hann', 4096)
for name, det, rdet in (('constant', _hip.DETREND_CONSTANT, 'constant'), ('fast', _hip.DETREND_CONSTANT_FAST, 'constant'), ('none', _hip.DETREND_NONE, False)):
    ulps, means = [], []
    for seed in range(12):
        x = R.synth_iq(4096, 100 + seed)
        ref = R.welch_np(x, fs=1.0, window=w, nperseg=4096, noverlap=2048, nfft=4096, detrend=rdet)[1]
        plan = ctx.welch_plan(4096, window=w, detrend=det, kernel=_hip.KERNEL_TUNED)
        plan.set_tuning('ws')
        got = plan.exec(x).astype(np.float64)
        assert plan.last_recipe().startswith('kernel=welch4096:ws '), plan.last_recipe()
        plan.close()
        ulps.append(np.max(np.abs(np.sqrt(got) - np.sqrt(ref))) / np.sqrt(ref.max()) * 2.0 ** 23)
        means.append(np.mean(np.abs(got - ref) / ref))
    print('welch4096ws one-segment rows, detrend %-8s: amplitude error %.2f ulp of the peak (worst of 12 seeds), mean relative power error %.2e'
          % (name, max(ulps), np.mean(means)))
ctx.close()
