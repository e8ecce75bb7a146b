"""savgol_apply_strided_multi_batch_f32 on the GPU: several record fields from one pass.

THE TWIN CHECK.  Every call is made twice: once as the multi call, once -- on a bit-for-bit copy of the buffers -- as the single
savgol_apply_strided_batch_f32_ex calls it stands for, in the caller's order.  The WHOLE buffers must then be equal bit for bit: the written fields
(so NaN positions coincide), the fields nobody writes, the slack between `count` records and the channel pitch, and guard rows in front of and behind
both arrays.  No tolerance anywhere.  Before every call _route is held to the rule restated in tests/strided_multi_rule.py, twice (the second call must
change nothing); the last test prints how many calls took a fused launch and asserts that the count is the rule's.  One case per half-window group of
the kernel objects is also held to the fp64 oracle under the project's one rule (bar32 / normwise / check), so that the twins cannot both be wrong.

Shapes: the smallest at which the kernel can go wrong -- count = 2n + 1 (one partial tile, the edge windows meet), 2048 + 2n + 3 (a second tile of
three records), 5000 (three tiles), once 70001; 1 to 4 channels; pitch with and without slack; records of 8, 12, 16, 20, 32 and 64 bytes; 2, 3, 4 jobs
(one launch), 5 and 7 (several launches, 5 with a last group of one), 16 on 64-byte records."""
import numpy as np
import pytest

from tests import strided_multi_rule as rule
from tests._util import check, normwise
from tests.test_gpu_1d import bar32

pytestmark = pytest.mark.gpu

REF, CLE, AWARE = 1, 16, 32
GUARD = 256                                         # floats in front of and behind each array
MIX = ((2, 0, 1.0), (3, 1, 0.5), (4, 2, 0.5), (4, 0, 1.0), (3, 1, 1.0), (2, 2, 1.0), (1, 0, 1.0), (2, 1, 0.25))      # (poly_order, derivative, time_step)
TALLY = {"calls": 0, "fused_calls": 0, "fused_launches": 0, "predicted_calls": 0, "predicted_launches": 0}


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert sg.device_count() > 0, sg.last_error()
    return torch


_filters = {}


def filt(sg, n, m, d, dt=1.0, boundary=0):
    """filters kept alive for the whole module"""
    key = (n, m, d, dt, boundary)
    if key not in _filters:
        _filters[key] = sg.Filter(n, m, d, dt, boundary)
    return _filters[key]


def mix(sg, n, count, boundary=None):
    """`count` filters of half window n: smoothing and derivatives, time steps != 1; boundary None = a different mode per job (ignored by default flags)"""
    specs = [s for s in MIX if s[0] < 2 * n + 1]
    return [filt(sg, n, *specs[k % len(specs)], boundary=(k % 4 if boundary is None else boundary)) for k in range(count)]


def as_int(torch, t):
    return t.view(torch.int32)


def twin(sg, torch, jobs, rec, ch, count, slack=0, two=True, flags=0, seed=1, poke=None, expect=None, stream=None):
    """jobs: [(Filter, in_offset, out_offset)] in bytes.  Runs the multi call and its twin, asserts route and bit equality of the whole buffers.
    Returns (the input array as it was, the multi call's output array, the route); arrays are numpy [ch, count + slack, rec / 4] views of the body."""
    L = sg.lib()
    recs = count + slack
    body = ch * recs * rec // 4
    rng = np.random.default_rng(seed)
    host = [rng.standard_normal(2 * GUARD + body).astype(np.float32) for _ in range(2 if two else 1)]
    if poke is not None:
        poke(host[0][GUARD:GUARD + body].reshape(ch, recs, rec // 4))
    mine = [torch.from_numpy(h).cuda() for h in host]
    theirs = [torch.from_numpy(h).cuda() for h in host]
    pitch = recs * rec

    def grids(bufs):
        return bufs[0].data_ptr() + 4 * GUARD, bufs[-1].data_ptr() + 4 * GUARD

    d_in, d_out = grids(mine)
    call = ([(f.n, int(f.ptr.contents.config.boundary), d_in + i, d_out + o) for f, i, o in jobs], rec, pitch, rec, pitch, ch, count, flags)
    want = rule.launches(*call)
    for _ in range(2):                              # a second _route call changes nothing
        got = sg.apply_strided_multi_batch_route(jobs, d_in, rec, pitch, d_out, rec, pitch, ch, count, flags)
        assert got == want, (got, want, sg.last_error())
    if expect is not None:
        assert want == expect, (want, expect)
    sg.apply_strided_multi_batch(jobs, d_in, rec, pitch, d_out, rec, pitch, ch, count, flags, stream=stream)
    t_in, t_out = grids(theirs)
    for f, i, o in jobs:
        rc = L.savgol_apply_strided_batch_f32_ex(f.ptr, t_in, rec, i, pitch, t_out, rec, o, pitch, ch, count, flags, None)
        assert rc == 0, sg.last_error()
    torch.cuda.synchronize()
    for a, b in zip(mine, theirs):
        same = torch.equal(as_int(torch, a), as_int(torch, b))
        if not same:
            bad = (as_int(torch, a) != as_int(torch, b)).nonzero().flatten().cpu().numpy()
            raise AssertionError(f"{len(bad)} words differ from the single calls, the first at float {bad[0] - GUARD} of the body "
                                 f"(record bytes {rec}, pitch {pitch}, count {count}, channels {ch}, jobs {[(f.n, i, o) for f, i, o in jobs]}, flags {flags:#x})")
    TALLY["calls"] += 1
    TALLY["fused_calls"] += got > 0
    TALLY["fused_launches"] += got
    TALLY["predicted_calls"] += want > 0
    TALLY["predicted_launches"] += want
    out = mine[-1].cpu().numpy()
    # the guards are the host's words still, and something was written
    assert np.array_equal(out[:GUARD].view(np.uint32), host[-1][:GUARD].view(np.uint32)) and np.array_equal(out[-GUARD:].view(np.uint32), host[-1][-GUARD:].view(np.uint32))
    assert not np.array_equal(out.view(np.uint32), host[-1].view(np.uint32))
    shape = (ch, recs, rec // 4)
    return host[0][GUARD:GUARD + body].reshape(shape), out[GUARD:GUARD + body].reshape(shape), got


def counts(n):
    """(channels, count, slack)"""
    return ((2, 2 * n + 1, 3), (3, 2048 + 2 * n + 3, 0), (4, 5000, 1), (1, 2048 + 2 * n + 3, 2))


FLAG_SETS = ((0, None), (CLE, None), (AWARE, 1), (AWARE, 3), (AWARE | CLE, 2), (AWARE, 0))       # (flags, the boundary every filter carries; None = mixed)


@pytest.mark.parametrize("n", (1, 5, 13, 32))
@pytest.mark.parametrize("rec", (8, 12, 16, 20, 32, 64))
def test_into_a_second_array(sg, torch_gpu, n, rec):
    """field k -> field k of a second array of the same shape: 2, 3, 4 jobs (one launch), 5 and 7 (two launches), every flag word"""
    F = rec // 4
    for k, (flags, boundary) in enumerate(FLAG_SETS):
        for njobs in (2, 3, 4, 5, 7):
            if njobs > F:
                continue
            ch, count, slack = counts(n)[(k + njobs) % 4]
            fs = mix(sg, n, njobs, boundary)
            jobs = [(fs[j], 4 * ((j * 3) % F), 4 * j) for j in range(njobs)]                   # inputs permuted, some shared where 3 divides F
            twin(sg, torch_gpu, jobs, rec, ch, count, slack, True, flags, seed=100 * n + rec + k, expect=(njobs + 2) // 4 if njobs != 5 else 1)


@pytest.mark.parametrize("n", (1, 5, 13, 32))
@pytest.mark.parametrize("rec", (12, 16, 20, 32, 64))
def test_into_other_fields_of_the_same_records(sg, torch_gpu, n, rec):
    """the in-place array-of-structs layout: the first fields of every record into its last fields (16-byte records: fields 0, 1 -> 2, 3)"""
    F = rec // 4
    for k, (flags, boundary) in enumerate(FLAG_SETS):
        for njobs in (2, 3, 4, 5, 7):
            n_in = max(1, F - njobs)                                                           # input fields [0, n_in), outputs the last njobs fields
            if F - njobs < 1:
                continue
            ch, count, slack = counts(n)[(k + njobs + 1) % 4]
            fs = mix(sg, n, njobs, boundary)
            jobs = [(fs[j], 4 * (j % n_in), 4 * (F - njobs + j)) for j in range(njobs)]
            src, out, _ = twin(sg, torch_gpu, jobs, rec, ch, count, slack, False, flags, seed=200 * n + rec + k, expect=(njobs + 2) // 4 if njobs != 5 else 1)
            assert np.array_equal(src[:, :, :F - njobs].view(np.uint32), out[:, :, :F - njobs].view(np.uint32))       # the input fields stay


@pytest.mark.parametrize("n", range(1, 33))
def test_every_half_window(sg, torch_gpu, n):
    """one kernel per half window: value, first and second derivative (one time step != 1) of field 0 into fields 1, 2, 3 of the same 16-byte records"""
    fs = [filt(sg, n, 2, 0), filt(sg, n, 2, 1, 0.5), filt(sg, n, 2, 2)]
    twin(sg, torch_gpu, [(fs[j], 0, 4 * (j + 1)) for j in range(3)], 16, 2, 2048 + 2 * n + 3, 0, False, 0, seed=n, expect=1)


@pytest.mark.parametrize("n", (1, 5, 13, 32))
def test_three_derivatives_of_one_field_and_the_same_filter_twice(sg, torch_gpu, n):
    fs = [filt(sg, n, 2, 0), filt(sg, n, 2, 1, 0.5), filt(sg, n, 2, 2)]
    for flags, two in ((0, False), (CLE, True), (AWARE, False)):
        for ch, count, slack in counts(n):
            twin(sg, torch_gpu, [(fs[j], 4, 4 * (j + 2)) for j in range(3)], 20, ch, count, slack, two, flags, seed=300 + n, expect=1)
    for ch, count, slack in counts(n):
        _, out, _ = twin(sg, torch_gpu, [(fs[1], 0, 4), (fs[1], 0, 8)], 12, ch, count, slack, False, CLE, seed=400 + n, expect=1)
        assert np.array_equal(out[:, :count, 1].view(np.uint32), out[:, :count, 2].view(np.uint32))     # the same filter twice: equal outputs


def test_sixteen_jobs_on_64_byte_records_and_a_long_channel(sg, torch_gpu):
    fs = mix(sg, 13, 16, 0)
    twin(sg, torch_gpu, [(fs[j], 4 * ((5 * j) % 16), 4 * j) for j in range(16)], 64, 2, 5000, 1, True, 0, seed=16, expect=4)
    fs = mix(sg, 5, 4)
    twin(sg, torch_gpu, [(fs[j], 4 * j, 16 + 4 * j) for j in range(4)], 32, 1, 70001, 0, False, 0, seed=17, expect=1)      # 35 tiles of one channel


def test_every_fallback_class_is_the_sequential_single_calls(sg, torch_gpu):
    """each class of call the rule does not fuse, once: _route == 0 and the bits of the single calls in order"""
    a, b, c = filt(sg, 5, 2, 0), filt(sg, 5, 3, 1, 0.5), filt(sg, 5, 4, 2)
    cases = (("a misaligned input field", [(a, 2, 8), (b, 4, 12)], 16, False, 0),
             ("output on an input field", [(a, 0, 8), (b, 8, 12)], 16, False, 0),
             ("output on its own input field", [(a, 0, 0), (b, 4, 12)], 16, False, 0),
             ("a read-after-write chain", [(a, 0, 4), (b, 4, 8), (c, 8, 12)], 16, False, 0),
             ("two jobs, one output field: the later wins", [(a, 0, 8), (b, 4, 8)], 16, False, 0),
             ("mixed half windows", [(a, 0, 8), (filt(sg, 6, 2, 0), 4, 12)], 16, False, 0),
             ("mixed boundary under BOUNDARY_AWARE", [(a, 0, 8), (filt(sg, 5, 2, 0, 1.0, 1), 4, 12)], 16, False, AWARE),
             ("REFERENCE_SUMMATION", [(a, 0, 8), (b, 4, 12)], 16, False, REF),
             ("a record size outside the table", [(a, 0, 0), (b, 4, 4)], 24, True, 0),
             ("one job", [(b, 4, 12)], 16, False, 0))
    for label, jobs, rec, two, flags in cases:
        for ch, count, slack in ((3, 2048 + 13, 1), (2, 13, 0)):
            _, _, route = twin(sg, torch_gpu, jobs, rec, ch, count, slack, two, flags, seed=500, expect=0)
            assert route == 0, label


@pytest.mark.parametrize("flags,boundary", ((0, 0), (AWARE, 1), (AWARE, 3), (AWARE, 2)))
@pytest.mark.parametrize("n", (5, 32))
def test_special_values(sg, torch_gpu, n, flags, boundary):
    """NaN, +-Inf, -0.0 and an all-zero channel in the interior, in a halo and in an edge window: the fused call's words are the single calls'"""
    count = 2048 + 2 * n + 3
    spots = (n // 2, 2 * n, 1000, 2048 - n, 2048 - 1, 2048, 2048 + n - 1, count - 2 * n - 1, count - 2)      # edge windows, interior, both halos of the tile seam

    def poke(v):
        v[0, :, 0] = 0.0                                                   # an all-zero channel of field 0 ...
        v[0, 500:600, 0] = -0.0                                            # ... with a stretch of negative zeros
        for k, s in enumerate(spots):
            v[1, s, 0] = (np.nan, np.inf, -np.inf, -0.0)[k % 4]
            v[2, s, 1] = (np.inf, -0.0, np.nan, -np.inf)[k % 4]
        v[3, :, 1] = -0.0

    fs = mix(sg, n, 4, boundary)
    src, out, _ = twin(sg, torch_gpu, [(fs[0], 0, 8), (fs[1], 4, 12), (fs[2], 0, 16), (fs[3], 4, 20)], 24 + 8, 4, count, 1, False, flags, seed=600 + n, poke=poke, expect=1)
    assert np.isnan(out[1, :count, 2]).any() and np.isnan(out[2, :count, 3]).any() and not np.isnan(out[0, :count, 2]).any()
    assert not out[0, :count, 2].any()                                     # zeros in, zeros out


@pytest.mark.parametrize("n,m,d", ((5, 2, 0), (16, 3, 1), (25, 4, 0), (32, 4, 2)))
def test_fused_outputs_against_the_fp64_oracle(sg, sgo, torch_gpu, n, m, d):
    """one case per half-window group of the kernel objects under the project's one rule, as test_strided_two_fields_of_the_same_records holds the single
    call: fields 0, 1 -> 2, 3 of the same 16-byte records, polynomial edges whatever config.boundary says"""
    fs = [filt(sg, n, m, d, 1.0, 2), filt(sg, n, 2, 0, 1.0, 1)]
    for ch, count, slack in ((3, 5000, 0), (2, 2 * n + 1, 3), (4, 2048 + 2 * n + 3, 1)):
        src, out, route = twin(sg, torch_gpu, [(fs[0], 0, 8), (fs[1], 4, 12)], 16, ch, count, slack, False, 0, seed=700 + n, expect=1)
        for (fm, fd), fi, fo in (((m, d), 0, 2), ((2, 0), 1, 3)):
            o = sgo.Filter(n, fm, fd, 1.0, 0)
            ref = o.apply_f64(src[:, :count, fi].astype(np.float64))
            check(normwise(out[:, :count, fo], ref), bar32(o, src[:, :count, fi], ref), (n, fm, fd, ch, count, fi, fo))


def test_graph_capture_and_replay(sg, torch_gpu):
    """after one warm-up call a fused call only enqueues: captured on one stream and replayed, it writes the eager call's words"""
    torch = torch_gpu
    n, ch, count, rec = 13, 3, 5000, 32
    fs = mix(sg, n, 5)
    jobs = [(fs[j], 4 * (j % 3), 12 + 4 * j) for j in range(5)]           # a launch of four and a single call
    pitch = count * rec
    x = torch.randn(ch * count * rec // 4, dtype=torch.float32, device="cuda")
    want = x.clone()
    assert sg.apply_strided_multi_batch_route(jobs, want, rec, pitch, want, rec, pitch, ch, count) == 1
    sg.apply_strided_multi_batch(jobs, want, rec, pitch, want, rec, pitch, ch, count)        # eager, and the warm-up
    torch.cuda.synchronize()
    out = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            sg.apply_strided_multi_batch(jobs, out, rec, pitch, out, rec, pitch, ch, count, stream=s)
    out.copy_(x)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(as_int(torch, out), as_int(torch, want)) and not torch.equal(as_int(torch, out), as_int(torch, x))


def test_zz_how_many_calls_took_a_fused_launch():
    """runs last in this file: the tally of every twin check above"""
    print(f"\nstrided multi: {TALLY['calls']} calls, {TALLY['fused_calls']} fused ({TALLY['fused_launches']} fused launches), "
          f"{TALLY['calls'] - TALLY['fused_calls']} as single calls; the rule predicted {TALLY['predicted_calls']} / {TALLY['predicted_launches']}")
    assert TALLY["fused_calls"] == TALLY["predicted_calls"] and TALLY["fused_launches"] == TALLY["predicted_launches"]
    if TALLY["calls"] > 100:                                               # the whole file ran, not one selected test: both routes were taken
        assert TALLY["fused_calls"] >= 100 and TALLY["calls"] - TALLY["fused_calls"] >= 20
