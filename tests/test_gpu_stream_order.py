"""The stream-ordering contract of include/ce_metrics.h (above ce_ctx_create_on_stream), on caller-owned streams and on the
library's own stream reached through Context.stream.

Method (tests/stream_hold.py): the context's stream is HELD - a bounded run of device-to-device copies is enqueued on it
first - so that whatever the test enqueues behind the hold is still pending when the next host call is made.  A fence the
library forgot between its streams (the metric chains' ev_fork / ev_join, SSIMULACRA2's ev_prep / ev_done, Butteraugli's
ev_ba_fork / ev_ba_join, ce_flush_uploads, ce_order_write's waits on ev_run and on an inline write, ce_upload_table) then
shows as the scores of the wrong images, bit for bit, instead of passing because every kernel finishes within a millisecond.

Expected values come from the blocking path on the session's context - a fresh batch, host uploads, run - which the rest of
the suite pins to the oracle; one pair per shape is compared with the oracle here as well.  The three image sets A, B and C
differ in every compared field of every pair (checked first), so no stale read can hide.

Power condition: a case that holds a stream asserts, right after the asynchronous call under test returns, that the stream
is still busy ("hold too short" otherwise); a blocking reader asserts with an event pair that hold + copy took at least the
hold's target.  The hold is 25 x the event-timed duration of one warmed all-metrics launch of the batch under test, at
least 20 ms, and the test asserts it stays under the 200 ms ceiling.

Hardware queues.  HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (4 where the process does not ask for
more), and a stream runs behind whatever waits in its queue.  Such a dependency orders MORE than the library asked for, so it
can hide a missing fence but never fake one.  Two cases are shaped by it:
 - The control (a producer on a stream that is not the context's) launches DSSIM + PSNR, which stays on one stream, and
   takes a new producer stream until one does not share that stream's queue: that one returns set A's scores.
 - An all-metrics launch parks a waiting packet in every one of four queues, so an upload that follows it waits with or
   without ce_order_write's wait for ev_run.  Group C therefore runs the upload-route writers a second time against a
   one-stream launch, on a batch whose upload stream was first SEEN to run beside the held stream (scenario_write).

The profiling modes (ce_prof_enable 1 and 2) enqueue like any launch - ce_prof_begin records events, only ce_prof_enable /
ce_prof_get drain the stream - so they carry the power condition too.  A warmed ce_batch_launch returns while the stream is
held in every case here; of the writers, the upload route returns late when it needs a staging buffer again whose last
image is still queued behind the launch (the third image of a burst), which the header states.

Out of reach: the rebuild of the pair table and the work lists (ce_upload_table's wait for ev_run) against a still-running
EARLIER launch of the same batch.  A second launch overwrites the first one's scores, so nothing the ABI returns can tell
whether the first one read the new table; no hook is invented for it.

torch: its default stream has handle 0, which means "own stream" to ce_ctx_create_on_stream and cannot be adopted; a
torch.cuda.Stream() can, when torch and the library share one HIP runtime in the process (the case is skipped otherwise).

Measured on an MI355X (every case prints its own, pytest -s): one 256 MiB device-to-device copy 0.098 - 0.106 ms; a warmed
all-metrics launch of 4 pairs 0.21 - 0.33 ms at either shape, so 25 launches are 5 - 8 ms and every hold is the 20 ms floor:
235 - 256 copies, sized for 1.25 x 20 ms; hold + copies measured around the blocking readers 25.0 - 25.3 ms.  With the
wait for ev_run taken out of ce_order_write the one-stream upload cases and the child process fail, with the wait for
ev_fork taken out of ce_batch_launch every forked reader of group B fails - wrong scores each time, no fault.
"""
import ctypes as C
import dataclasses
import importlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reference_reuse_cases as R  # noqa: E402
import stream_hold as SH  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = R.SHAPES  # 72 x 40 and 130 x 67
N_REFS, N_PAIRS = 2, 4
BIND = [1, 0, 0, 1]
SETS = {"A": (500, 30, 9), "B": (600, 47, 11), "C": (700, 62, 7)}  # reference seed, first quality, quality step
REL_TOL = 1e-4  # the suite's bar against the oracle (tests/test_gpu_parity.py); PSNR is exact


# ---- values as comparable bit patterns ---------------------------------------------------------------------------------

def canon(x):
    if isinstance(x, np.ndarray):
        return (x.shape, str(x.dtype), x.tobytes())
    if isinstance(x, float):
        return struct.pack("<d", x)
    if dataclasses.is_dataclass(x):
        return tuple(canon(getattr(x, f.name)) for f in dataclasses.fields(x))
    if isinstance(x, C.Structure):
        return tuple(R.bits([x])[0])
    if isinstance(x, (list, tuple)):
        return tuple(canon(v) for v in x)
    return x


# ---- the image sets ----------------------------------------------------------------------------------------------------

class ImageSet:
    def __init__(self, ce, wl, w, h, name):
        seed, q0, dq = SETS[name]
        self.name, self.w, self.h = name, w, h
        self.refs8 = [wl.make_reference(w, h, seed + r) for r in range(N_REFS)]
        self.tests8 = [wl.distort(self.refs8[BIND[k]], q0 + dq * k) for k in range(N_PAIRS)]
        self.by_kind = {kind: ([R.convert(ce, kind, a) for a in self.refs8], [R.convert(ce, kind, a) for a in self.tests8])
                        for kind in ("rgb8", "linear")}
        self.staged = {}

    def images(self, kind):
        return self.by_kind[kind]

    def on_device(self, H, kind):
        """(references, tests) staged in device memory, complete"""
        if kind not in self.staged:
            refs, tests = self.by_kind[kind]
            self.staged[kind] = ([H.stage(a) for a in refs], [H.stage(a) for a in tests])
        return self.staged[kind]


_sets = {}


def image_set(ce, wl, w, h, name):
    if (w, h, name) not in _sets:
        _sets[(w, h, name)] = ImageSet(ce, wl, w, h, name)
    return _sets[(w, h, name)]


def rgba(rgb8):
    a = np.ascontiguousarray(rgb8).reshape(-1, 3)
    return np.concatenate([a, np.full((a.shape[0], 1), 255, np.uint8)], axis=1)


# ---- a batch under test ------------------------------------------------------------------------------------------------

class Rig:
    """A batch of 2 references and 4 pairs on `ctx`, its slab addresses (fetched once and kept, so references written through
    them are announced with references_changed()) and the context's stream."""

    def __init__(self, ce, H, ctx, kind, w, h):
        self.ce, self.H, self.ctx, self.kind, self.w, self.h = ce, H, ctx, kind, w, h
        self.b = ctx.batch_linear(w, h, N_REFS, N_PAIRS) if kind == "linear" else ce.Batch(ctx, w, h, N_REFS, N_PAIRS)
        self.ref_slab, self.test_slab = self.b.reference_slab, self.b.test_slab
        self.S = ctx.stream
        self.img_bytes = w * h * (12 if kind == "linear" else 3)
        self.extra = {}  # further batches and device buffers a reader or a writer keeps

    def fill_host(self, s):
        refs, tests = s.images(self.kind)
        for r in range(N_REFS):
            self.b.set_reference(r, refs[r])
        for k in range(N_PAIRS):
            self.b.set_test(k, BIND[k], tests[k])

    def copy_async(self, s, stream, tests_only=None):
        """set `s` from its staged copies into the slabs on `stream`, nothing synchronised"""
        refs, tests = s.on_device(self.H, self.kind)
        if tests_only is None:
            for r in range(N_REFS):
                self.H.copy_to_slot(stream, self.ref_slab, r, refs[r])
        for k in (range(N_PAIRS) if tests_only is None else tests_only):
            self.H.copy_to_slot(stream, self.test_slab, k, tests[k])

    def batch(self, key, w, h):
        """a further batch of the same kind on the same context, pairs bound as BIND, made on first use"""
        if key not in self.extra:
            b = self.ctx.batch_linear(w, h, N_REFS, N_PAIRS) if self.kind == "linear" else self.ce.Batch(self.ctx, w, h, N_REFS, N_PAIRS)
            for k in range(N_PAIRS):
                b.bind_pair(k, BIND[k])
            self.extra[key] = b
        return self.extra[key]

    def launch_ms(self):
        """the event-timed duration of one all-metrics launch of the batch, warmed by one before it"""
        self.b.launch(N_PAIRS, self.ce.MetricConfig.all())
        self.b.collect(N_PAIRS)
        e0, e1 = self.H.event(), self.H.event()
        e0.record(self.S)
        self.b.launch(N_PAIRS, self.ce.MetricConfig.all())
        e1.record(self.S)
        self.b.collect(N_PAIRS)
        e1.synchronize()
        return e0.ms_until(e1)

    def close(self):
        for v in self.extra.values():
            if hasattr(v, "close"):
                v.close()
        self.extra = {}
        self.b.close()


def hold_for(rig, what, before=None):
    """hold the rig's stream for 25 warmed launches (at least 20 ms), with the event `before` recorded ahead of the hold;
    prints both measured values"""
    ms = rig.launch_ms()
    target = SH.hold_ms_for(ms)
    assert target <= SH.HOLD_MAX_MS / SH.SAFETY, f"a launch of {ms:.3f} ms asks for a hold over the ceiling"
    rig.ctx.synchronize()
    if before is not None:
        before.record(rig.S)
    k = rig.H.hold(rig.S, target)
    print(f"[stream-order] {what} {rig.kind} {rig.w}x{rig.h}: launch {ms:.3f} ms, hold target {target:.1f} ms = {k} copies of "
          f"{rig.H.copy_ms:.3f} ms")
    return target


# ---- readers: (result, stream busy when the asynchronous call returned | None for a blocking reader) ------------------------

def reader_launch(cfg_of, prof=0, **kw):
    def read(rig):
        ce = rig.ce
        if prof:
            rig.ctx._check(ce.lib().ce_prof_enable(rig.ctx._h, prof))
        try:
            rig.b.launch(N_PAIRS, cfg_of(ce), **kw)
            busy = rig.H.busy(rig.S)
            return R.bits(rig.b.collect(N_PAIRS)), busy
        finally:
            if prof:
                rig.ctx._check(ce.lib().ce_prof_enable(rig.ctx._h, 0))
    return read


def read_heuristics(rig):
    return canon([rig.b.image_heuristics(0, N_REFS), rig.b.image_heuristics(0, N_PAIRS, tests=True)]), None


def read_hdr(rig):
    maps, _ = rig.b.delta_e_itp_maps(0, N_PAIRS)
    return canon([rig.b.hdr_fidelity(N_PAIRS), maps]), None


def read_copy_device(rig):
    """both slabs moved into a second batch by Context.copy_device ("ordered like a kernel of this context"), scored there"""
    other = rig.batch("same", rig.w, rig.h)
    rig.ctx.copy_device(other.reference_slab, rig.ref_slab, N_REFS * rig.img_bytes)  # fetching the address says: references change
    rig.ctx.copy_device(other.test_slab, rig.test_slab, N_PAIRS * rig.img_bytes)
    other.launch(N_PAIRS, rig.ce.MetricConfig.all())
    busy = rig.H.busy(rig.S)
    return R.bits(other.collect(N_PAIRS)), busy


def read_resample(rig):
    """the viewing simulation's step: resampled on the device into a smaller batch, scored there"""
    small = rig.batch("small", rig.w * 2 // 3, rig.h * 2 // 3)
    rig.b.resample_pairs_into(small, N_REFS, N_PAIRS)
    small.launch(N_PAIRS, rig.ce.MetricConfig.all())
    busy = rig.H.busy(rig.S)
    return R.bits(small.collect(N_PAIRS)), busy


READERS = {
    "all": ("rgb8", reader_launch(lambda ce: ce.MetricConfig.all())),
    "all_linear": ("linear", reader_launch(lambda ce: ce.MetricConfig.all())),
    "dssim": ("rgb8", reader_launch(lambda ce: ce.MetricConfig(dssim=True))),
    "ssimulacra2": ("rgb8", reader_launch(lambda ce: ce.MetricConfig(ssimulacra2=True))),
    "butteraugli": ("rgb8", reader_launch(lambda ce: ce.MetricConfig(butteraugli=True))),
    "psnr": ("rgb8", reader_launch(lambda ce: ce.MetricConfig(psnr=True))),
    "dssim_psnr": ("rgb8", reader_launch(lambda ce: ce.MetricConfig(dssim=True, psnr=True))),
    "dssim_linear": ("linear", reader_launch(lambda ce: ce.MetricConfig(dssim=True))),
    "xyb_roundtrip": ("rgb8", reader_launch(lambda ce: ce.MetricConfig.all().with_xyb_roundtrip())),
    "prof_forked": ("rgb8", reader_launch(lambda ce: ce.MetricConfig.all(), prof=2)),
    "prof_serial": ("rgb8", reader_launch(lambda ce: ce.MetricConfig.all(), prof=1)),
    "heuristics": ("rgb8", read_heuristics),
    "hdr_fidelity": ("linear", read_hdr),
    "copy_device": ("rgb8", read_copy_device),
    "resample": ("rgb8", read_resample),
    "resample_linear": ("linear", read_resample),
}

_want = {}


def want_read(ce, wl, H, gpu_ctx, reader_name, w, h, set_name):
    """what a reader returns on the blocking path: the session's context, a fresh batch, host uploads, everything synchronised"""
    key = ("read", reader_name, w, h, set_name)
    if key not in _want:
        kind, read = READERS[reader_name]
        rig = Rig(ce, H, gpu_ctx, kind, w, h)
        try:
            rig.fill_host(image_set(ce, wl, w, h, set_name))
            gpu_ctx.synchronize()
            _want[key] = read(rig)[0]
        finally:
            rig.close()
    return _want[key]


# ---- writers: prepare (may synchronise) and apply (must not wait for the stream) ----------------------------------------

def write_fmt_rgba8(rig, s):
    for k in range(N_PAIRS):  # the upload-stream route: wide staging, the ingest kernel on up_stream
        rig.b.set_test_fmt(k, BIND[k], rgba(s.tests8[k]), rig.ce.PIXEL_RGBA8)


def write_set_test(rig, s):
    for k in range(N_PAIRS):  # the inline route of a small batch: on the context's stream
        rig.b.set_test(k, BIND[k], s.images(rig.kind)[1][k])


def write_set_reference(rig, s):
    for r in range(N_REFS):
        rig.b.set_reference(r, s.images(rig.kind)[0][r])


def prepare_yuv(rig, s):
    """4:4:4 planes in device memory, complete: the three channels of set s's test images read as Y', Cb and Cr"""
    if ("yuv", s.name) not in rig.extra:
        images = []
        for k in range(N_PAIRS):
            planes = [rig.H.stage(np.ascontiguousarray(s.tests8[k].reshape(rig.h, rig.w, 3)[:, :, c])) for c in range(3)]
            images.append((planes, rig.ce.YuvImage([p.address for p in planes], subsampling=rig.ce.YUV_444, memory=rig.ce.MEM_DEVICE,
                                                   pitches=[rig.w] * 3)))
        rig.extra[("yuv", s.name)] = images


def write_yuv_device(rig, s):
    for k, (_planes, img) in enumerate(rig.extra[("yuv", s.name)]):
        rig.b.set_test_yuv(k, BIND[k], img)


def write_cicp(rig, s):
    for k in range(N_PAIRS):
        rig.b.set_test_cicp(k, BIND[k], s.tests8[k].reshape(rig.h, rig.w, 3), rig.ce.ColourDescription.DISPLAY_P3)


def write_memset(rig, s):
    """the caller's own writes of both slabs on the context's stream"""
    rig.H.memset_async(rig.S, rig.ref_slab, 0x40, N_REFS * rig.img_bytes)
    rig.H.memset_async(rig.S, rig.test_slab, 0x90, N_PAIRS * rig.img_bytes)
    rig.b.references_changed()


def prepare_resample(rig, s):
    if ("big", s.name) not in rig.extra:
        W, H_ = rig.w * 3 // 2, rig.h * 3 // 2
        big = rig.batch(("big", s.name), W, H_)
        wl = importlib.import_module("codec-eval_amd.workloads")
        src = image_set(rig.ce, wl, W, H_, s.name)
        refs, tests = src.images(rig.kind)
        for r in range(N_REFS):
            big.set_reference(r, refs[r])
        for k in range(N_PAIRS):
            big.set_test(k, BIND[k], tests[k])
        rig.ctx.synchronize()


def write_resample(rig, s):
    rig.extra[("big", s.name)].resample_pairs_into(rig.b, N_REFS, N_PAIRS)


WRITERS = {
    "fmt_rgba8": ("rgb8", None, write_fmt_rgba8),
    "set_test": ("rgb8", None, write_set_test),
    "set_reference": ("rgb8", None, write_set_reference),
    "yuv_device": ("rgb8", prepare_yuv, write_yuv_device),
    "cicp_linear": ("linear", None, write_cicp),
    "memset": ("rgb8", None, write_memset),
    "resample": ("rgb8", prepare_resample, write_resample),
}


def one_stream_config(ce, kind):
    """(the reader's name, a launch that stays on the context's stream: DSSIM and PSNR have no stream of their own)"""
    return ("dssim_linear", ce.MetricConfig(dssim=True)) if kind == "linear" else ("dssim_psnr", ce.MetricConfig(dssim=True, psnr=True))


def want_written(ce, wl, H, gpu_ctx, writer_name, w, h, one_stream=False):
    """the scores of a fresh batch on the blocking path that received set B, then the writer with set C"""
    key = ("write", writer_name, w, h, one_stream)
    if key not in _want:
        kind, prepare, write = WRITERS[writer_name]
        cfg = one_stream_config(ce, kind)[1] if one_stream else ce.MetricConfig.all()
        rig = Rig(ce, H, gpu_ctx, kind, w, h)
        try:
            rig.fill_host(image_set(ce, wl, w, h, "B"))
            if prepare:
                prepare(rig, image_set(ce, wl, w, h, "C"))
            write(rig, image_set(ce, wl, w, h, "C"))
            _want[key] = R.bits(rig.b.run(N_PAIRS, cfg))
        finally:
            rig.close()
    return _want[key]


# ---- the two scenarios, shared with the child process -------------------------------------------------------------------

def scenario_read(ce, wl, H, ctx, reader_name, w, h):
    """Group B: the slabs hold A; then hold, B copied into the slabs on the context's stream, the reader - with no host
    synchronisation.  -> (the reader's result over A, synchronised; its result behind the held producer)"""
    kind, read = READERS[reader_name]
    A, B = image_set(ce, wl, w, h, "A"), image_set(ce, wl, w, h, "B")
    B.on_device(H, kind)
    rig = Rig(ce, H, ctx, kind, w, h)
    try:
        rig.fill_host(A)
        got_a = read(rig)[0]  # warms every allocation, table and stream of the path
        e0, e1 = H.event(), H.event()
        target = hold_for(rig, "read " + reader_name, before=e0)  # synchronises, then holds
        rig.copy_async(B, rig.S)
        e1.record(rig.S)
        rig.b.references_changed()
        got_b, busy = read(rig)
        if busy is None:  # a blocking reader: it waited for the whole hold
            e1.synchronize()
            spent = e0.ms_until(e1)
            print(f"[stream-order] read {reader_name}: blocking; hold + copies took {spent:.1f} ms")
            assert spent >= target, f"hold too short: {spent:.1f} ms of the {target:.1f} ms asked for"
        else:
            print(f"[stream-order] read {reader_name}: stream busy when the call returned: {busy}")
            assert busy, "hold too short: the stream was idle when the call under test returned"
        return got_a, got_b
    finally:
        ctx.synchronize()
        rig.close()


def upload_stream_runs_beside(rig, B):
    """Does the batch's upload stream run while the context's stream is held?  HIP multiplexes streams onto
    GPU_MAX_HW_QUEUES hardware queues (4 unless the process asks for more) and a stream that shares a queue with a held one
    waits behind it, whatever the library does.  Seen through the ABI alone: the staging of the upload route has two
    buffers, so a third upload returns only once the first one's conversion has run on the upload stream."""
    rig.b.run(N_PAIRS, rig.ce.MetricConfig(dssim=True))  # behind the inline writes: the uploads below wait for nothing of the library's
    image = B.images(rig.kind)[1][0] if rig.kind == "linear" else rgba(B.tests8[0])

    def three_uploads():
        for _ in range(3):
            if rig.kind == "linear":
                rig.b.set_test(0, BIND[0], image)  # float images take the upload route
            else:
                rig.b.set_test_fmt(0, BIND[0], image, rig.ce.PIXEL_RGBA8)
    three_uploads()  # makes the staging
    rig.ctx.synchronize()
    rig.H.hold(rig.S, SH.HOLD_MIN_MS)
    three_uploads()
    beside = rig.H.busy(rig.S)
    rig.ctx.synchronize()
    return beside


def scenario_write(ce, wl, H, ctx, writer_name, w, h, one_stream=False):
    """Group C: the batch holds B; then hold, launch L1, the writer with set C, collect L1, run L2.
    -> (L1's scores, L2's scores)

    one_stream: L1 is a launch that stays on the context's stream, on a batch whose upload stream was seen to run beside
    that stream.  An all-metrics launch parks a waiting packet on every one of four hardware queues, and whatever is
    enqueued after it on ANY stream then runs behind it: the fence between the launch and the upload stream
    (ce_order_write's wait for ev_run) cannot be told from its absence there."""
    kind, prepare, write = WRITERS[writer_name]
    B, Cset = image_set(ce, wl, w, h, "B"), image_set(ce, wl, w, h, "C")
    cfg = one_stream_config(ce, kind)[1] if one_stream else ce.MetricConfig.all()
    rigs = []
    try:
        while True:
            rig = Rig(ce, H, ctx, kind, w, h)
            rigs.append(rig)  # kept: a new stream goes to the hardware queue with the fewest streams, so they spread
            rig.fill_host(B)
            if not one_stream or upload_stream_runs_beside(rig, B):
                break
            assert len(rigs) < 8, "hold without power: no batch whose upload stream runs beside the context's stream"
        if one_stream:
            print(f"[stream-order] write {writer_name}: batch {len(rigs)} has an upload stream that runs beside the context's stream")
        if prepare:
            prepare(rig, Cset)
        write(rig, Cset)  # warms the writer's staging and streams
        ctx.synchronize()
        rig.fill_host(B)
        warm = R.bits(rig.b.run(N_PAIRS, cfg))
        hold_for(rig, "write " + writer_name)
        rig.b.launch(N_PAIRS, cfg)
        busy = H.busy(rig.S)
        assert busy, "hold too short: the stream was idle when the warmed launch returned (or the launch waits for it)"
        write(rig, Cset)
        print(f"[stream-order] write {writer_name}: stream busy after the writer returned: {H.busy(rig.S)}")
        first = R.bits(rig.b.collect(N_PAIRS))
        second = R.bits(rig.b.run(N_PAIRS, cfg))
        assert warm == first, "the held launch does not return what the same launch returned on an idle stream"
        return first, second
    finally:
        ctx.synchronize()
        for rig in rigs:
            rig.close()


# ---- fixtures -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def H(ce, gpu_ctx):
    h = SH.holder(ce)
    print(f"[stream-order] one 256 MiB device-to-device copy: {h.copy_ms:.3f} ms")
    return h


@pytest.fixture(scope="module")
def streams(ce, H, gpu_ctx):
    """the contexts under test: on a caller-owned non-blocking stream, and one with a stream of its own"""
    s = H.stream_create(SH.STREAM_NON_BLOCKING)
    caller, own = ce.Context(0, stream=s), ce.Context(0)
    assert caller.stream == s and own.stream not in (0, s)
    yield {"caller": caller, "own": own}
    caller.close()
    own.close()
    assert H.stream_synchronize(s) == 0 and H.stream_destroy(s) == 0


# ---- the inputs ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SHAPES)
def test_inputs_differ_in_every_field_and_match_the_oracle(ce, workloads, oracle, gpu_ctx, H, w, h):
    """A condition on the inputs: the expected results of A, B and C differ pairwise in every compared field of every pair,
    for every reader and writer - and the blocking path itself stands on the oracle for one pair per shape."""
    for name, (kind, _read) in READERS.items():
        got = [want_read(ce, workloads, H, gpu_ctx, name, w, h, s) for s in "ABC"]
        if name in ("heuristics", "hdr_fidelity"):
            assert got[0] != got[1] and got[1] != got[2] and got[0] != got[2], name
            continue
        valid = got[0][0][1]
        fields = [2 + i for i, m in enumerate((ce.METRIC_DSSIM, ce.METRIC_SSIMULACRA2, ce.METRIC_BUTTERAUGLI, ce.METRIC_PSNR)) if valid & m]
        assert fields, name
        for k in range(N_PAIRS):
            assert all(g[k][0] == 0 and g[k][1] == valid for g in got), (name, k)
            for f in fields:
                assert len({g[k][f] for g in got}) == 3, f"{name}: pair {k} field {f} does not tell A, B and C apart"
    b_all = want_read(ce, workloads, H, gpu_ctx, "all", w, h, "B")
    for name in WRITERS:
        second = want_written(ce, workloads, H, gpu_ctx, name, w, h)
        ref = want_read(ce, workloads, H, gpu_ctx, "all_linear" if WRITERS[name][0] == "linear" else "all", w, h, "B")
        changed = range(N_PAIRS)
        for k in changed:
            assert second[k][0] == 0
            differs = [f for f in range(2, 6) if second[k][f] != ref[k][f]]
            assert len(differs) >= 3, f"{name}: pair {k} after the writer is too close to B's"
    # the oracle, at the suite's bars, for pair 0 of set B
    B = image_set(ce, workloads, w, h, "B")
    r, t = B.refs8[BIND[0]], B.tests8[0]
    s = [struct.unpack("<d", struct.pack("<Q", v))[0] for v in b_all[0][2:]]  # dssim, ssimulacra2, butteraugli, psnr
    close = lambda got, want, floor=1.0: abs(got - want) <= REL_TOL * max(abs(want), floor)  # noqa: E731
    assert s[3] == oracle.psnr(r, t, w, h)
    assert close(s[1], oracle.ssimulacra2(r, t, w, h, 1))
    assert close(s[0], oracle.dssim(r, t, w, h), floor=1e-6)
    assert close(s[2], oracle.butteraugli(r, t, w, h)[0])


# ---- A. a context on a caller-owned stream computes the same bits -------------------------------------------------------

def everything(ce, wl, ctx):
    """Every kind of call the library has, on `ctx`: name -> bit patterns."""
    out = {}
    cfg = ce.MetricConfig.all()
    for (w, h) in SHAPES:
        tag = f"{w}x{h}:"
        B, Cset = image_set(ce, wl, w, h, "B"), image_set(ce, wl, w, h, "C")
        r8, t8 = B.refs8[0], B.tests8[1]
        out[tag + "calculate_metrics"] = canon(ctx.calculate_metrics(r8, t8, w, h, cfg))
        out[tag + "xyb_roundtrip"] = canon(ctx.xyb_roundtrip(r8, w, h))
        dm = ctx.calculate_butteraugli_diffmap(r8, t8, w, h)
        out[tag + "butteraugli_diffmap"] = canon([dm.score, dm.diffmap])
        out[tag + "image_heuristics"] = canon(ctx.image_heuristics(t8, w, h))
        batches = {}
        for kind in ("rgb8", "deep", "linear"):
            if kind == "deep":
                b = ctx.batch_deep(w, h, N_REFS, N_PAIRS, 10, 10)
                deep = lambda a: (np.ascontiguousarray(a).reshape(-1, 3).astype(np.uint16) * 4 + np.arange(w * h, dtype=np.uint16)[:, None] % 3)  # noqa: E731
                refs, tests = [deep(a) for a in B.refs8], [deep(a) for a in B.tests8]
            else:
                b = ctx.batch_linear(w, h, N_REFS, N_PAIRS) if kind == "linear" else ce.Batch(ctx, w, h, N_REFS, N_PAIRS)
                refs, tests = B.images(kind)
            batches[kind] = b
            for r in range(N_REFS):
                b.set_reference(r, refs[r])
            for k in range(N_PAIRS):
                b.set_test(k, BIND[k], tests[k])
            out[tag + kind + ":run"] = R.bits(b.run(N_PAIRS, cfg, butteraugli_diffmap=True, ssimulacra2_maps=True))
            out[tag + kind + ":butteraugli_diffmaps"] = canon(b.butteraugli_diffmaps(0, N_PAIRS))
            out[tag + kind + ":dssim_ssim_maps"] = canon(list(b.dssim_ssim_maps(1, 0, N_PAIRS)))
            out[tag + kind + ":ssimulacra2_maps"] = canon(list(b.ssimulacra2_maps(1, 1, ce.SSIM2_MAP_ARTIFACT, 0, N_PAIRS)))
        out[tag + "batch_heuristics"] = canon(batches["rgb8"].image_heuristics(0, N_PAIRS, tests=True))
        out[tag + "hdr_fidelity"] = canon(batches["linear"].hdr_fidelity(N_PAIRS))
        small = ce.Batch(ctx, w * 2 // 3, h * 2 // 3, N_REFS, N_PAIRS)
        batches["rgb8"].resample_pairs_into(small, N_REFS, N_PAIRS)
        out[tag + "resample_then_run"] = R.bits(small.run(N_PAIRS, cfg))
        small.close()
        for b in batches.values():
            b.close()
        handle = ce.ReferenceHandle(ctx, r8, w, h)
        out[tag + "compare_many"] = canon(handle.compare_many([B.tests8[1], B.tests8[2], Cset.tests8[0]], cfg))
        handle.close()
    # 20 pairs over both shapes from page-locked memory: 20 images per shape, so ce_eval_batch opens its second DMA stream
    items, keep = [], []
    for (w, h) in SHAPES:
        n = w * h * 3
        slab = ctx.host_buffer(20 * n)
        keep.append(slab)
        for i in range(10):
            s = image_set(ce, wl, w, h, "ABC"[i % 3])
            rv, tv = slab[2 * i * n:(2 * i + 1) * n], slab[(2 * i + 1) * n:(2 * i + 2) * n]
            rv[:] = s.refs8[BIND[i % N_PAIRS]].reshape(-1)
            tv[:] = s.tests8[i % N_PAIRS].reshape(-1)
            items.append((rv, tv, w, h))
    out["eval_batch"] = R.bits(ctx.eval_batch(items, cfg))
    del items, keep
    return out


_everything_want = {}


def check_everything(ce, wl, gpu_ctx, ctx):
    if not _everything_want:
        _everything_want.update(everything(ce, wl, gpu_ctx))
    got = everything(ce, wl, ctx)
    assert got.keys() == _everything_want.keys()
    for name in got:
        assert got[name] == _everything_want[name], f"{name} differs on the caller-owned stream"


@pytest.mark.parametrize("flags", [SH.STREAM_NON_BLOCKING, SH.STREAM_DEFAULT], ids=["non_blocking", "default_flags"])
def test_caller_stream_computes_the_same_bits_and_stays_the_callers(ce, workloads, gpu_ctx, H, flags):
    s = H.stream_create(flags)
    ctx = ce.Context(0, stream=s)
    try:
        assert ctx.stream == s
        check_everything(ce, workloads, gpu_ctx, ctx)
        ctx.synchronize()
    finally:
        ctx.close()
    # ce_ctx_destroy honours own_stream: the stream still works and is the caller's to destroy
    assert H.hold(s, SH.HOLD_MIN_MS) > 0
    assert H.busy(s)
    assert H.stream_synchronize(s) == 0
    assert not H.busy(s)
    assert H.stream_destroy(s) == 0


def test_two_contexts_on_one_caller_stream(ce, workloads, gpu_ctx, H):
    s = H.stream_create(SH.STREAM_NON_BLOCKING)
    c1, c2 = ce.Context(0, stream=s), ce.Context(0, stream=s)
    try:
        cfg = ce.MetricConfig.all()
        for (w, h) in SHAPES:
            r1, r2 = Rig(ce, H, c1, "rgb8", w, h), Rig(ce, H, c2, "rgb8", w, h)
            try:
                r1.fill_host(image_set(ce, workloads, w, h, "A"))
                r2.fill_host(image_set(ce, workloads, w, h, "B"))
                for _ in range(2):  # interleaved launches, collected in reverse order
                    r1.b.launch(N_PAIRS, cfg)
                    r2.b.launch(N_PAIRS, cfg)
                got2, got1 = R.bits(r2.b.collect(N_PAIRS)), R.bits(r1.b.collect(N_PAIRS))
                assert got1 == want_read(ce, workloads, H, gpu_ctx, "all", w, h, "A")
                assert got2 == want_read(ce, workloads, H, gpu_ctx, "all", w, h, "B")
            finally:
                r1.close()
                r2.close()
    finally:
        c1.close()
        c2.close()
    assert H.stream_synchronize(s) == 0 and H.stream_destroy(s) == 0


def test_stream_zero_means_an_own_stream(ce):
    """NULL = own stream (include/ce_metrics.h): the legacy default stream - torch's default stream has this handle - is not
    adopted."""
    for ctx in (ce.Context(0, stream=0), ce.Context(0, stream=None)):
        try:
            assert ctx.stream != 0
        finally:
            ctx.close()
    h = C.c_void_p()
    assert ce.lib().ce_ctx_create_on_stream(0, None, C.byref(h)) == 0 and h.value
    assert ce.lib().ce_ctx_stream(h)
    ce.lib().ce_ctx_destroy(h)


def hip_runtimes_mapped():
    with open("/proc/self/maps") as f:
        return sorted({os.path.realpath(line.split()[-1]) for line in f if "libamdhip64" in line})


def test_torch_stream(ce, workloads, gpu_ctx, H):
    """A torch.cuda.Stream() as the context's stream - where torch and the library share one HIP runtime.  A torch wheel that
    ships a libamdhip64.so of its own maps a second one: its stream handles mean nothing to the library's runtime."""
    import importlib.util

    reason = "torch maps a HIP runtime of its own ({} copies of libamdhip64 in the process): its stream handles mean nothing to the library's runtime"
    spec = importlib.util.find_spec("torch")
    assert spec is not None and spec.origin
    own = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(own) and os.path.realpath(own) not in hip_runtimes_mapped():
        pytest.skip(reason.format(len(hip_runtimes_mapped()) + 1))  # known without paying for the import
    import torch

    mapped = hip_runtimes_mapped()
    if len(mapped) != 1:
        pytest.skip(reason.format(len(mapped)))
    stream = torch.cuda.Stream()
    ctx = ce.Context(0, stream=stream.cuda_stream)
    try:
        assert ctx.stream == stream.cuda_stream
        for (w, h) in SHAPES:
            got_a, got_b = scenario_read(ce, workloads, H, ctx, "all", w, h)
            assert got_a == want_read(ce, workloads, H, gpu_ctx, "all", w, h, "A")
            assert got_b == want_read(ce, workloads, H, gpu_ctx, "all", w, h, "B")
    finally:
        ctx.close()
    stream.synchronize()


# ---- B. work enqueued on the context's stream before a call is seen by the call -----------------------------------------

@pytest.mark.parametrize("reader_name", list(READERS))
@pytest.mark.parametrize("owner", ["caller", "own"])
def test_a_call_sees_what_the_stream_holds_before_it(ce, workloads, gpu_ctx, H, streams, owner, reader_name):
    for (w, h) in SHAPES:
        got_a, got_b = scenario_read(ce, workloads, H, streams[owner], reader_name, w, h)
        assert got_a == want_read(ce, workloads, H, gpu_ctx, reader_name, w, h, "A"), "the reader on an idle stream"
        want_b = want_read(ce, workloads, H, gpu_ctx, reader_name, w, h, "B")
        assert got_b != got_a
        assert got_b == want_b, ("the reader ran ahead of the copies enqueued before it: set A's result" if got_b == got_a
                                 else "neither A's nor B's result")


@pytest.mark.parametrize("owner", ["caller", "own"])
def test_a_launch_sees_three_routes_at_once(ce, workloads, gpu_ctx, H, streams, owner):
    """The references through set_reference (inline: on the context's stream, behind the hold), pairs 0, 2 and 3 through
    the slab on the context's stream, pair 1 through set_test_fmt(RGBA8) on the batch's upload stream: one launch sees all."""
    ctx, cfg = streams[owner], ce.MetricConfig.all()
    for (w, h) in SHAPES:
        A, B = image_set(ce, workloads, w, h, "A"), image_set(ce, workloads, w, h, "B")
        B.on_device(H, "rgb8")
        rig = Rig(ce, H, ctx, "rgb8", w, h)
        try:
            rig.fill_host(A)
            rig.b.set_test_fmt(1, BIND[1], rgba(A.tests8[1]), ce.PIXEL_RGBA8)
            assert R.bits(rig.b.run(N_PAIRS, cfg)) == want_read(ce, workloads, H, gpu_ctx, "all", w, h, "A")
            hold_for(rig, "mixed routes")
            for r in range(N_REFS):
                rig.b.set_reference(r, B.refs8[r])
            rig.copy_async(B, rig.S, tests_only=(0, 2, 3))
            rig.b.set_test_fmt(1, BIND[1], rgba(B.tests8[1]), ce.PIXEL_RGBA8)
            rig.b.launch(N_PAIRS, cfg)
            assert H.busy(rig.S), "hold too short: the stream was idle when the launch returned"
            assert R.bits(rig.b.collect(N_PAIRS)) == want_read(ce, workloads, H, gpu_ctx, "all", w, h, "B")
        finally:
            ctx.synchronize()
            rig.close()


def test_control_another_stream_is_not_waited_for(ce, workloads, gpu_ctx, H, streams):
    """The same producer on a stream that is not the context's: the launch does not wait for it (the header says so for
    CE_MEM_DEVICE planes) and returns set A's scores - which also shows that the method detects a missing dependency.  The
    stale reads are ordinary loads of the slabs.

    HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues, and a stream that shares a queue with a busy one waits
    for it: a dependency nobody asked for, which the library cannot prevent.  So the launch here is DSSIM + PSNR, which
    stays on the context's stream alone, and the producer's stream is made up to eight times, each kept until the end - the
    runtime gives a new stream the hardware queue with the fewest streams on it, so streams that stay alive spread over
    the queues.  Every attempt must return exactly A's scores (not waited for) or exactly B's (the shared queue); the
    first that does not share the context's queue returns A's and ends the case."""
    ctx, name = streams["caller"], "dssim_psnr"
    cfg = ce.MetricConfig(dssim=True, psnr=True)
    for (w, h) in SHAPES:
        A, B = image_set(ce, workloads, w, h, "A"), image_set(ce, workloads, w, h, "B")
        want_a, want_b = (want_read(ce, workloads, H, gpu_ctx, name, w, h, s) for s in "AB")
        B.on_device(H, "rgb8")
        rig = Rig(ce, H, ctx, "rgb8", w, h)
        outcomes, others = [], []
        try:
            for _attempt in range(8):
                other = H.stream_create(SH.STREAM_NON_BLOCKING)
                others.append(other)
                try:
                    rig.fill_host(A)
                    assert R.bits(rig.b.run(N_PAIRS, cfg)) == want_a
                    ms = rig.launch_ms()
                    ctx.synchronize()
                    H.hold(other, SH.hold_ms_for(ms))
                    rig.copy_async(B, other)
                    rig.b.references_changed()
                    rig.b.launch(N_PAIRS, cfg)
                    got = R.bits(rig.b.collect(N_PAIRS))
                    busy = H.busy(other)
                    H.stream_synchronize(other)
                    assert got in (want_a, want_b), "neither A's nor B's scores"
                    outcomes.append("A" if got == want_a else "B")
                    if got == want_a:
                        assert busy, "hold too short: the producer had finished when the launch was collected"
                    rig.b.references_changed()
                    assert R.bits(rig.b.run(N_PAIRS, cfg)) == want_b, "the producer's copies, once synchronised"
                finally:
                    H.stream_synchronize(other)
                    ctx.synchronize()
                if outcomes[-1] == "A":
                    break
            print(f"[stream-order] control {w}x{h}: launches against producers on other streams returned {outcomes}")
            assert outcomes[-1] == "A", "every launch waited for a stream that is not the context's"
        finally:
            for other in others:
                assert H.stream_destroy(other) == 0
            rig.close()


# ---- C. a held launch is not disturbed by what follows it ---------------------------------------------------------------

@pytest.mark.parametrize("writer_name", list(WRITERS))
@pytest.mark.parametrize("owner", ["caller", "own"])
def test_a_held_launch_is_not_disturbed_by_a_later_write(ce, workloads, gpu_ctx, H, streams, owner, writer_name):
    """Also the contract "launch returns without the final wait": the warmed launch returns while the stream is held."""
    kind = WRITERS[writer_name][0]
    for (w, h) in SHAPES:
        first, second = scenario_write(ce, workloads, H, streams[owner], writer_name, w, h)
        want_first = want_read(ce, workloads, H, gpu_ctx, "all_linear" if kind == "linear" else "all", w, h, "B")
        want_second = want_written(ce, workloads, H, gpu_ctx, writer_name, w, h)
        assert first == want_first, "the write that followed the launch reached the images the launch was still to read"
        assert second == want_second, "the next launch does not see the write"


@pytest.mark.parametrize("writer_name", ["fmt_rgba8", "yuv_device", "cicp_linear"])
@pytest.mark.parametrize("owner", ["caller", "own"])
def test_a_held_launch_on_one_stream_is_not_disturbed_by_an_upload(ce, workloads, gpu_ctx, H, streams, owner, writer_name):
    """The upload-stream writers against a launch that leaves the upload stream's hardware queue free (scenario_write): here
    only ce_order_write's wait for ev_run keeps the upload behind the launch."""
    kind = WRITERS[writer_name][0]
    for (w, h) in SHAPES:
        first, second = scenario_write(ce, workloads, H, streams[owner], writer_name, w, h, one_stream=True)
        assert first == want_read(ce, workloads, H, gpu_ctx, one_stream_config(ce, kind)[0], w, h, "B"), \
            "the upload that followed the launch reached the images the launch was still to read"
        assert second == want_written(ce, workloads, H, gpu_ctx, writer_name, w, h, one_stream=True), "the next launch does not see the write"


# ---- D. the partly forked schedule, which only a process of its own can select ------------------------------------------

def child_main():
    """Runs in the child: group B's all-metrics reader and group C's first writer on a caller-owned stream."""
    ce = importlib.import_module("codec-eval_amd")
    wl = importlib.import_module("codec-eval_amd.workloads")
    H = SH.holder(ce)
    s = H.stream_create(SH.STREAM_NON_BLOCKING)
    ctx = ce.Context(0, stream=s)
    out = []
    for (w, h) in SHAPES:
        got_a, got_b = scenario_read(ce, wl, H, ctx, "all", w, h)
        first, second = scenario_write(ce, wl, H, ctx, next(iter(WRITERS)), w, h)
        out.append([got_a, got_b, first, second, list(scenario_write(ce, wl, H, ctx, next(iter(WRITERS)), w, h, one_stream=True))])
    ctx.close()
    assert H.stream_synchronize(s) == 0 and H.stream_destroy(s) == 0
    print(json.dumps(out))


def test_partly_forked_schedule_in_a_child_process(ce, workloads, gpu_ctx, H):
    env = dict(os.environ)
    env["CE_METRIC_STREAMS"] = "fork:dssim,ba"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_stream_order as T; T.child_main()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    writer_name = next(iter(WRITERS))
    as_lists = lambda rows: [list(row) for row in rows]  # noqa: E731
    for (w, h), (got_a, got_b, first, second, on_one_stream) in zip(SHAPES, got):
        assert on_one_stream[0] == as_lists(want_read(ce, workloads, H, gpu_ctx, "dssim_psnr", w, h, "B"))
        assert on_one_stream[1] == as_lists(want_written(ce, workloads, H, gpu_ctx, writer_name, w, h, one_stream=True))
        assert got_a == as_lists(want_read(ce, workloads, H, gpu_ctx, "all", w, h, "A"))
        assert got_b == as_lists(want_read(ce, workloads, H, gpu_ctx, "all", w, h, "B"))
        assert first == as_lists(want_read(ce, workloads, H, gpu_ctx, "all", w, h, "B"))
        assert second == as_lists(want_written(ce, workloads, H, gpu_ctx, writer_name, w, h))
