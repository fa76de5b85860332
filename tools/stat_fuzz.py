#!/usr/bin/env python3
"""The seeded random-shape cases of the per-bin statistic families (tests/stat_fuzz_cases.py: eleven families x nine sizes x
three classes a seed) for other seeds than the suite's, with the suite's checks (stat_fuzz_cases.run_case: the float64
oracle of every stream's own samples at the family's gates, guards, spare rows, the input read back, the host form's bits).
usage: stat_fuzz.py [--out file] [--timeout s] [seeds ...]      (default: seeds 1 ... 5; exits 1 on any failure)
Every seed runs in a fresh child process of its own under `timeout`, one after the other; a seed that fails, or a child that
dies or runs out of time, ends the run.  A committed run: profiles/stat_fuzz.txt."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'gr-ofdm_tools_amd'), ROOT):
    sys.path.insert(0, p)


def child(seed):
    """every case of one seed on one context -> exit status 1 if any failed"""
    import stat_fuzz_cases as S
    from ofdm_tools import _hip
    from stat_support import POWERS
    ctx = _hip.Context(0)
    failed, count, t0 = 0, 0, time.time()
    for family in S.FAMILIES:
        worst, walked = {}, False
        for nfft in POWERS:
            for c in S.cases(family, nfft, seed):
                count += 1
                try:
                    S.check_domain(c)
                    recipe, shares = S.run_case(ctx, _hip, c, say=lambda text: None)
                except AssertionError as e:
                    failed += 1
                    print('seed %d FAILED %s: %s' % (seed, S.shape_text(c), str(e)[:600]), flush=True)
                    continue
                except _hip.HipError as e:      # a refusal of an in-domain case, or an error of the device: nothing more runs on it
                    print('seed %d FAILED %s: %s - the seed ends here' % (seed, S.shape_text(c), str(e)[:600]), flush=True)
                    return 1
                walked = walked or (c.cls == 'C' and S.walks(c, recipe))
                for k, v in shares.items():
                    if v > worst.get(k, (0.0,))[0]:
                        worst[k] = (v, S.shape_text(c), recipe)
        for k, (v, text, recipe) in sorted(worst.items()):
            print('seed %d %-7s worst %-6s %.3f of its gate  [%s] [%s]' % (seed, family, k, v, text, recipe), flush=True)
        print('seed %d %-7s a class-C launch with runs of unequal length: %s' % (seed, family, 'yes' if walked else 'no'), flush=True)
    print('seed %d: %d cases, %d failed, %.0f s' % (seed, count, failed, time.time() - t0), flush=True)
    return 1 if failed else 0


def main(argv):
    out, limit, seeds = None, 900, []
    args = list(argv)
    while args:
        a = args.pop(0)
        if a == '--child':
            return child(int(args.pop(0)))
        if a == '--out':
            out = args.pop(0)
        elif a == '--timeout':
            limit = int(args.pop(0))
        else:
            seeds.append(int(a))
    text = []
    for seed in seeds or [1, 2, 3, 4, 5]:
        p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--child', str(seed)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(p.stdout, end='', flush=True)
        text.append(p.stdout)
        if p.returncode != 0:
            text.append('seed %d: exit status %d - the run ends here\n' % (seed, p.returncode))
            print(text[-1], end='', flush=True)
            break
    if out:
        with open(out, 'w') as f:
            f.write(''.join(text))
    return 1 if p.returncode != 0 else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
