"""savgol_apply_strided_multi_batch_f32 against the single strided calls it replaces, interleaved in one process (tools, not product).

Shapes: records of 2, 3, 4, 5, 8 and 16 floats at the sizes of tools/time_strided.py (2048 x 2^19 ... 1024 x 2^17 records); half windows 5, 16, 32;
each record size in two layouts -- "two": field k of one array into field k of a second array of the same shape, "same": the first fields of every
record into its last fields (in place; an 8-byte record has no room for two outputs beside an input, so that layout starts at 12 bytes) -- and with
K = 2, 4 and as many jobs as the layout holds (every field for "two", half the fields for "same") where these differ.

Method: SETS fresh buffer sets, the earlier ones still allocated; on each, after a warm-up of both sides on the first, REPS rounds of [the multi call,
the K single calls] enqueued back to back with device events around each side and ONE synchronise at the end of the shape, so the chip stays busy
throughout.  Once per shape, before timing, the outputs of the two sides are compared bit for bit at that size.  Per shape: the median ms of both sides
over all sets and rounds, the ratio, the byte bound (K x for one launch; K / groups where the jobs take several launches, a last group of one being a
single call), the record bytes a perfect one-pass call moves (every group reads the input records and writes -- read-modify-write, or merged into lines
just read -- the output records) over the fused time as a fraction of 8 TB/s, the route, and the SPREAD OF THE SINGLE CALLS over the buffer sets in
this same run ((max - min) / median of the per-set medians): a ratio within that spread of 1 is level.

    python tools/time_strided_multi.py [half windows, default 5,16,32]        environment: SETS (5), REPS (3), SCALE (divides the record counts, 1)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

sg = load_package()
import torch

L = sg.lib()
NS = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "5,16,32").split(",")]
SETS, REPS, SCALE = int(os.environ.get("SETS", "5")), int(os.environ.get("REPS", "3")), int(os.environ.get("SCALE", "1"))
SHAPES = ((2, 2048, 1 << 19), (3, 2048, 1 << 18), (4, 2048, 1 << 18), (5, 1024, 1 << 18), (8, 1024, 1 << 18), (16, 1024, 1 << 17))       # (floats per record, channels, records)
MIX = ((4, 0, 1.0), (3, 1, 0.5), (4, 2, 0.5), (2, 0, 1.0))
PEAK = 8e12


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def layouts(rec):
    """[(layout, K, [(in field, out field)])]"""
    out = []
    for K in sorted({k for k in (2, 4, rec) if k <= rec}):
        out.append(("two", K, [(k, k) for k in range(K)]))
    for K in sorted({k for k in (2, 4, rec // 2) if 2 <= k <= rec - 1}):
        n_in = rec - K
        out.append(("same", K, [(k % n_in, rec - K + k) for k in range(K)]))
    return out


def timed(fn, stream_events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    stream_events.append((e0, e1))


print(f"# savgol_apply_strided_multi_batch_f32 vs the K single calls, interleaved; {SETS} buffer sets x {REPS} rounds, medians; {torch.cuda.get_device_name(0)}", flush=True)
for rec, ch, count in SHAPES:
    count //= SCALE
    pitch = count * rec * 4
    nrec = ch * count
    sets = []
    for s in range(SETS):                                                   # fresh sets, the earlier ones stay allocated
        sets.append((torch.randn((ch, count, rec), device="cuda"), torch.randn((ch, count, rec), device="cuda")))
    for n in NS:
        filters = [sg.Filter(n, m, d, dt, 0) for m, d, dt in MIX]
        for layout, K, fields in layouts(rec):
            jobs = [(filters[k % 4], 4 * i, 4 * o) for k, (i, o) in enumerate(fields)]

            def args(bufs):
                src, dst = bufs
                return (src, rec * 4, pitch, dst if layout == "two" else src, rec * 4, pitch, ch, count)

            def multi(bufs):
                sg.apply_strided_multi_batch(jobs, *args(bufs))

            def singles(bufs):
                a = args(bufs)
                for f, i, o in jobs:
                    rc = L.savgol_apply_strided_batch_f32_ex(f.ptr, a[0].data_ptr(), a[1], i, a[2], a[3].data_ptr(), a[4], o, a[5], ch, count, 0, None)
                    assert rc == 0, sg.last_error()

            route = sg.apply_strided_multi_batch_route(jobs, *args(sets[0]))
            groups = (K + 3) // 4 if route > 0 else K                      # launches that each move the records once (a last group of one included)
            # bit equality at this size, once (and the warm-up of both sides): two copies of set 0
            a = tuple(t.clone() for t in sets[0]); b = tuple(t.clone() for t in sets[0])
            multi(a); singles(b); torch.cuda.synchronize()
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), (rec, n, layout, K, "the multi call's words are not the single calls'")
            del a, b
            ev_m, ev_s = [], []
            for bufs in sets:
                for _ in range(REPS):
                    timed(lambda: multi(bufs), ev_m)
                    timed(lambda: singles(bufs), ev_s)
            torch.cuda.synchronize()
            tm = [e0.elapsed_time(e1) for e0, e1 in ev_m]
            ts = [e0.elapsed_time(e1) for e0, e1 in ev_s]
            per_set = [median(ts[s * REPS:(s + 1) * REPS]) for s in range(SETS)]
            spread = (max(per_set) - min(per_set)) / median(per_set)
            mm, ms = median(tm), median(ts)
            record_bytes = groups * 2 * rec * 4 * nrec
            print(f"rec {rec * 4:2d} B  n={n:2d}  {layout:4s}  K={K:2d}  route {route} ({'fused' if route else 'single calls'})  multi {mm:8.3f} ms  singles {ms:8.3f} ms  "
                  f"ratio {ms / mm:5.2f} (byte bound {K / groups:4.2f})  {nrec / mm / 1e6:7.1f} G records/s  record bytes {record_bytes / mm / 1e6:6.0f} GB/s = "
                  f"{record_bytes / mm / 1e-3 / PEAK * 100:4.1f} % of 8 TB/s  singles' spread over sets {spread * 100:4.1f} %", flush=True)
    del sets
    torch.cuda.empty_cache()
