#!/usr/bin/env python3
"""The seeded random-shape cases of the core Welch and CSD routes (tests/core_fuzz_cases.py: three classes for every route
of resolve_recipe() and every forced build) for other seeds than the suite's, with the suite's checks
(core_fuzz_cases.run_case: the predicted recipe, the float64 oracle of every stream's own samples at the project's gates,
guards, spare rows, the input read back, the host form's bits).
usage: core_fuzz.py [--out file] [seeds ...]      (default: seeds 1 ... 5; exits 1 on any failure)
One line per case with the worst share of its gate, a summary per route and seed at the end.  Every seed runs in this one
process on one context; a failed comparison is counted and the run goes on, a HIP error ends the run at once - nothing more
is started on a device that has reported one.  A committed run: profiles/core_fuzz.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'gr-ofdm_tools_amd'), ROOT):
    sys.path.insert(0, p)


def main(argv):
    import core_fuzz_cases as K
    from ofdm_tools import _hip
    out, seeds = None, []
    args = list(argv)
    while args:
        a = args.pop(0)
        if a == '--out':
            out = args.pop(0)
        else:
            seeds.append(int(a))
    seeds = seeds or [1, 2, 3, 4, 5]
    if out:
        open(out, 'w').close()

    def say(text):
        print(text, flush=True)
        if out:
            with open(out, 'a') as f:
                f.write(text + '\n')

    ctx = _hip.Context(0)
    failed, count, worst, t0, status = 0, 0, {}, time.time(), 0
    try:
        for seed in seeds:
            for route in K.routes():
                rid = K.route_id(route)
                for c in K.cases(route, seed):
                    count += 1
                    try:
                        K.check_domain(c)
                        ran = K.run_case(ctx, _hip, c, say=lambda text: None)
                    except AssertionError as e:
                        failed += 1
                        say('seed %d FAILED %s: %s' % (seed, K.shape_text(c), str(e)[:900]))
                        continue
                    except _hip.HipError as e:      # a refusal of an in-domain case, or an error of the device: nothing more runs on it
                        say('seed %d FAILED %s: %s - the run ends here' % (seed, K.shape_text(c), str(e)[:600]))
                        status = 1
                        return 1
                    share = max(v for _, shares in ran for v in shares.values())
                    walked = sum(K.walks(r, L) for (r, _), L in zip(ran, c.launches))
                    say('seed %d %s: %d launch%s, %d walking, worst %.3f of its gate' % (
                        seed, K.shape_text(c), len(ran), '' if len(ran) == 1 else 'es', walked, share))
                    if share > worst.get(rid, (0.0,))[0]:
                        worst[rid] = (share, seed, K.shape_text(c))
        for rid in K.DRAWN:
            if rid in worst:
                say('route %-44s worst %.3f of its gate  [seed %d: %s]' % ((rid,) + worst[rid]))
        say('seeds %s: %d cases, %d failed, %.0f s' % (' '.join(str(s) for s in seeds), count, failed, time.time() - t0))
        return 1 if failed else 0
    finally:
        if not status:
            ctx.close()


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
