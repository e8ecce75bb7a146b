"""Several builds of libsavgol_hip.so in ONE process, for the A/B tools (never rank builds across processes): load() binds a build with the
package's signatures, alternate() times one call per build in interleaved rounds, report() prints the medians and, where the first build is
listed a second time, the new-against-parent difference next to the parent-against-parent difference of the same run."""
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_loaded = set()


def package():
    from __graft_entry__ import load_package
    return load_package()


def load(path):
    """The C ABI of the build at `path`; a build that is listed twice is loaded twice (from a copy under another name)."""
    import torch  # noqa: F401  (its HIP runtime first, so that all builds share one copy)
    sg = package()
    real = os.path.realpath(path)
    if real in _loaded:
        real = tempfile.NamedTemporaryFile(suffix=".so", delete=False).name
        shutil.copy(path, real)
    _loaded.add(real)
    L = C.CDLL(real)
    for name, (res, args) in sg.SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def new_filter(L, n, m, d=0, dt=1.0, mode=0):
    cfg = package().SavgolConfig(n, m, d, dt, mode)
    f = L.savgol_create(C.byref(cfg))
    assert f, f"savgol_create rejected n={n} m={m} d={d}"
    return f


def alternate(calls, rounds):
    """calls: one function per build; returns one list of milliseconds per build (HIP events, the builds interleaved inside every round)."""
    import torch
    for fn in calls:
        fn()                                                   # warm-up: plans, tables, code objects
    torch.cuda.synchronize()
    ts = [[] for _ in calls]
    for _ in range(rounds):
        for fn, t in zip(calls, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return ts


def report(label, paths, ts):
    med = [statistics.median(t) for t in ts]
    for p, t, m in zip(paths, ts, med):
        print(f"{label:28s} {p:40s} median {m:.4f} ms  min {min(t):.4f}  max {max(t):.4f}", flush=True)
    if len(paths) == 3 and paths[0] == paths[2]:
        print(f"{label:28s} new - parent {med[1] - med[0]:+.4f} ms ({(med[1] / med[0] - 1) * 100:+.2f} %);  parent - parent {med[2] - med[0]:+.4f} ms "
              f"({(med[2] / med[0] - 1) * 100:+.2f} %)", flush=True)
