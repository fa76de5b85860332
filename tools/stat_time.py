"""What the timing tools of the per-bin statistics share (mtm_ftest_time, welch_sk_time, mtm_jackknife_time,
mtm_adaptive_time, welch_cyclic_time): the command line (`[reps] [--out FILE]` and the tool's own flags), a context on
torch's current stream, say(), whole steps timed with HIP events, the arms alternating after two warm-up steps each with
the median over the repetitions reported, the resource table of a statistic's kernel builds, and the file under profiles/.
A tool keeps its shapes, its arms and its tie-out line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gr-ofdm_tools_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from ofdm_tools import _hip  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

TONES = ((0.5, 0.1234), (0.05, -0.31), (2.0, 0.4071))


class Session(object):
    def __init__(self, default_out, reps=30, inner=1, flags=()):
        """default_out: the file under profiles/, or {flag: file} with None for no flag; inner: calls per timed window."""
        argv = sys.argv[1:]
        self.flags = set(f for f in flags if f in argv)
        if isinstance(default_out, dict):
            default_out = next((v for k, v in default_out.items() if k in self.flags), default_out[None])
        self.out_path = os.path.join(ROOT, 'profiles', default_out)
        if '--out' in argv:
            i = argv.index('--out')
            self.out_path = argv[i + 1]
            del argv[i:i + 2]
        args = [a for a in argv if not a.startswith('--')]
        self.reps, self.inner, self.lines = (int(args[0]) if args else reps), inner, []
        self.dev = torch.device('cuda', 0)
        self.stream = torch.cuda.current_stream(self.dev)
        self.ctx = _hip.Context(0, stream=self.stream.cuda_stream)
        self.library = 'library %s on %s' % (os.path.basename(_hip.LIB_PATH), self.ctx.device_name())

    def say(self, text):
        print(text, flush=True)
        self.lines.append(text)

    def timed(self, fn):
        """ms per call of one timed window"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        for _ in range(self.inner):
            fn()
        b.record(self.stream)
        b.synchronize()
        return a.elapsed_time(b) / self.inner

    def capture(self, n, seed=2026, tones=TONES, dc=0.1 + 0.05j):
        """n synthetic IQ samples on the device, as 2 n floats"""
        x = torch.empty(2 * n, dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self.ctx.synth_iq(x.data_ptr(), n, seed, tones, dc)
        return x

    def run_arms(self, cands):
        """cands: [(label, fn, plan)] -> {label: median ms}, {label: min ms}, {label: the plan's recipe after its warm-up}"""
        recipes = {}
        for label, fn, plan in cands:      # warm-up: workspaces, first launches
            fn()
            fn()
            recipes[label] = plan.last_recipe()
        torch.cuda.synchronize(self.dev)
        ms = {label: [] for label, _, _ in cands}
        for _ in range(self.reps):
            for label, fn, _ in cands:
                ms[label].append(self.timed(fn))
        return {k: float(np.median(v)) for k, v in ms.items()}, {k: float(min(v)) for k, v in ms.items()}, recipes

    def report(self, name, cands, width, first, n=None):
        """Times the arms and says the shape's block: one line per arm, its ratio to the first arm (`first`: what to call
        it), with n the samples per step behind the rate.  -> the medians"""
        med, low, recipes = self.run_arms(cands)
        self.say('')
        self.say(name)
        base = med[cands[0][0]]
        for label, _, _ in cands:
            v = med[label]
            rate = '  %8.0f Msamples/s' % (n / v / 1e3) if n else ''
            self.say('  %-*s %9.3f ms per %s (median of %d, min %.3f)%s  x%.2f of the %s   [%s]'
                     % (width, label, v, 'step' if n else 'call', self.reps, low[label], rate, v / base, first, recipes[label]))
        return med

    def finish(self, header, filters, width=64, key=None):
        """Closes the context, says the resource table of the kernels whose names hold one of `filters` - by transform length,
        or by key(name, length) - and writes the file."""
        import kernel_resources
        self.ctx.close()
        self.say('')
        ks = {n: v for n, v in kernel_resources.kernels(_hip.LIB_PATH).items() if any(f in n for f in filters)}
        self.say('%-*s %5s %5s %6s %9s' % (width, header, 'VGPR', 'SGPR', 'spills', 'scratch B'))

        def length(q):
            return int(q.split('<')[1].split(',')[0]) if '<' in q else 0
        for n in sorted(ks, key=(lambda q: key(q, length(q))) if key else length):
            k = ks[n]
            self.say('%-*s %5d %5d %6d %9d' % (width, n.split('(')[0], k['vgpr'] + k['agpr'], k['sgpr'], k['spill_vgpr'], k['scratch']))
        os.makedirs(os.path.dirname(os.path.abspath(self.out_path)), exist_ok=True)
        with open(self.out_path, 'w') as f:
            f.write('\n'.join(self.lines) + '\n')
