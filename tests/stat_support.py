"""What the suites of the per-bin statistics (test_welch_*, test_mtm*) share - a plain module, no fixtures: the Welch plan
of the GPU suites, a forced environment variable, a field of last_recipe, and the bodies of the surface tests and of the
no-scratch tests on the code objects of the built library."""
import contextlib
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))      # kernel_resources
FS = 2.5
POWERS = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)      # the sizes the taper-loop kernels are built for


def welch_plan(ctx, hip, nfft, nperseg=None, noverlap=0, detrend=True, scaling='density', fftshift=False, trim=0, db=False, fs=FS, **kw):
    """a Hann-windowed Welch plan as the statistics' GPU suites make it"""
    from test_median_gpu import SCALINGS, window
    nperseg = nfft if nperseg is None else nperseg
    return ctx.welch_plan(nfft, nperseg=nperseg, noverlap=noverlap, window=window('hann', nperseg),
                          detrend=hip.DETREND_CONSTANT if detrend else hip.DETREND_NONE, scaling=SCALINGS[scaling], fs=fs,
                          fftshift=fftshift, trim_bins=trim, db=db, **kw)


@contextlib.contextmanager
def forced_env(name, value):
    """the environment variable `name` reads `value` inside (None: left as it is) - a plan created inside reads it"""
    old = os.environ.get(name)
    if value is not None:
        os.environ[name] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def recipe_field(recipe, name):
    return int(recipe.split(' %s=' % name)[1].split()[0])


def check_surface(symbols, cls, methods, header_lines=()):
    """The entry points `symbols` are declared in the public header (with `header_lines` verbatim), have a ctypes signature,
    the methods on the class `cls` of ofdm_tools._hip, and - once the library is built - are exported."""
    from ofdm_tools import _hip
    header = open(os.path.join(ROOT, 'include', 'ofdm_tools_hip.h')).read()
    for name in symbols:
        assert 'int %s(' % name in header and name in _hip.SIGNATURES
    for line in header_lines:
        assert line in header
    for name in methods:
        assert hasattr(getattr(_hip, cls), name)
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    lib = _hip.load()
    for name in symbols:
        assert getattr(lib, name) is not None


def check_builds(kernel, builds, budget, extra_kernels=()):
    """The builds of the kernel template `kernel` in the code objects of the built library are exactly `builds` - the sizes
    (template argument 0), or (size, variant) pairs (arguments 0 and 2: the argument between them is the thread count) -,
    each of them and each of `extra_kernels` has no private segment and no spilled register, and a build of T threads keeps
    vgpr + agpr inside budget[T] (a thread count the budget leaves out is free; one it names has a build).  Prints a
    resource line per kernel -> [(template arguments, resources)] of the builds."""
    import kernel_resources
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    every = kernel_resources.kernels(_hip.LIB_PATH)
    start = re.compile(r'(?<![\w])%s<' % re.escape(kernel))
    found = []
    for n, v in sorted(every.items()):
        m = start.search(n)
        if m:
            text = n[m.end():].split('>')[0]
            args = tuple(t.strip() == 'true' if t.strip() in ('true', 'false') else int(t) for t in text.split(','))
            found.append(('%s<%s>' % (kernel, text), args, v))
    extra = [(e, None, v) for e in extra_kernels for n, v in sorted(every.items()) if re.search(r'(?<![\w])%s\b' % re.escape(e), n)]
    pair = builds and isinstance(builds[0], tuple)
    assert sorted((a[0], a[2]) if pair else a[0] for _, a, _ in found) == list(builds), [n for n, _, _ in found]
    assert len(extra) == len(extra_kernels), [n for n, _, _ in extra]
    for name, _, v in found + extra:
        print('%s: vgpr %d agpr %d sgpr %d scratch %d lds %d' % (name, v['vgpr'], v['agpr'], v['sgpr'], v['scratch'], v.get('lds', 0)))
    bad = {n: (v['scratch'], v['spill_vgpr'], v['spill_sgpr']) for n, _, v in found + extra
           if v['scratch'] or v['spill_vgpr'] or v['spill_sgpr']}
    assert not bad, bad
    assert set(budget) <= set(a[1] for _, a, _ in found), budget
    for name, a, v in found:
        assert v['vgpr'] + v['agpr'] <= budget.get(a[1], 1 << 30), (name, v)
    return [(a, v) for _, a, v in found]
