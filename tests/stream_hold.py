"""Holding a HIP stream for a bounded time, for tests/test_gpu_stream_order.py (a helper, not a test).

A stream is held by enqueueing k device-to-device copies between two scratch buffers of 256 MiB on it: plain copies, which
always finish - no host callback, no spinning kernel.  Whatever is enqueued behind them is still pending when the next
host call is made, so a dependency the library forgot shows as the scores of the wrong images.  One copy is timed once per
process with an event pair on an idle stream, and k follows from the time asked for.

Every HIP call goes through the library's own runtime handle (ce.lib()), as the suite's hipMalloc / hipMemcpy already do:
torch ships a libamdhip64.so of its own, and a stream or an event made by one copy of the runtime means nothing to the other.
"""
import ctypes as C
import math

import numpy as np

H2D, D2H, D2D = 1, 2, 3
STREAM_DEFAULT, STREAM_NON_BLOCKING = 0, 1  # hipStreamDefault, hipStreamNonBlocking
NOT_READY = 600  # hipErrorNotReady
SCRATCH_BYTES = 256 << 20
HOLD_FACTOR, HOLD_MIN_MS, HOLD_MAX_MS = 25.0, 20.0, 200.0
# k is sized for SAFETY x the time asked for, so that copies that run faster than they did when they were timed still hold
# the stream that long; hold_ms_for() leaves the room for it under HOLD_MAX_MS
SAFETY = 1.25


def hold_ms_for(launch_ms):
    """The hold for a batch whose warmed launch takes launch_ms: 25 launches, at least 20 ms; the caller asserts that this
    stays under the ceiling rather than have it cut."""
    return max(HOLD_FACTOR * launch_ms, HOLD_MIN_MS)


class DeviceBuffer:
    """hipMalloc'ed bytes, freed with the object"""

    def __init__(self, lib, nbytes):
        self.lib, self.ptr, self.nbytes = lib, C.c_void_p(), nbytes
        assert lib.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0

    @property
    def address(self):
        return self.ptr.value

    def __del__(self):
        if self.ptr:
            self.lib.hipFree(self.ptr)
            self.ptr = C.c_void_p()


class Event:
    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p()
        assert lib.hipEventCreate(C.byref(self.h)) == 0

    def record(self, stream):
        assert self.lib.hipEventRecord(self.h, C.c_void_p(stream)) == 0

    def synchronize(self):
        assert self.lib.hipEventSynchronize(self.h) == 0

    def ms_until(self, later):
        """milliseconds from this event to `later`, both complete"""
        ms = C.c_float()
        assert self.lib.hipEventElapsedTime(C.byref(ms), self.h, later.h) == 0
        return float(ms.value)

    def __del__(self):
        if self.h:
            self.lib.hipEventDestroy(self.h)
            self.h = C.c_void_p()


class Holder:
    """The scratch buffers, the calibration and every HIP call the stream-order tests make."""

    CALIBRATION_COPIES = 32

    def __init__(self, ce):
        self.ce, self.lib = ce, ce.lib()
        self.a, self.b = DeviceBuffer(self.lib, SCRATCH_BYTES), DeviceBuffer(self.lib, SCRATCH_BYTES)
        s = self.stream_create(STREAM_NON_BLOCKING)
        try:
            e0, e1 = Event(self.lib), Event(self.lib)
            self._copies(s, 8)  # the first copies pay for page mapping and clocks
            self.stream_synchronize(s)
            times = []
            for _ in range(2):
                e0.record(s)
                self._copies(s, self.CALIBRATION_COPIES)
                e1.record(s)
                e1.synchronize()
                times.append(e0.ms_until(e1) / self.CALIBRATION_COPIES)
            self.copy_ms = min(times)  # the faster run: the larger k
        finally:
            self.stream_destroy(s)
        assert 0.0 < self.copy_ms < HOLD_MAX_MS / 4, self.copy_ms

    # -- streams
    def stream_create(self, flags):
        s = C.c_void_p()
        assert self.lib.hipStreamCreateWithFlags(C.byref(s), C.c_uint(flags)) == 0 and s.value
        return s.value

    def stream_destroy(self, stream):
        return self.lib.hipStreamDestroy(C.c_void_p(stream))

    def stream_synchronize(self, stream):
        rc = self.lib.hipStreamSynchronize(C.c_void_p(stream))
        assert rc == 0, rc
        return rc

    def busy(self, stream):
        """true while work enqueued on `stream` has not finished"""
        rc = self.lib.hipStreamQuery(C.c_void_p(stream))
        assert rc in (0, NOT_READY), rc
        return rc == NOT_READY

    def event(self):
        return Event(self.lib)

    # -- the hold
    def _copies(self, stream, k):
        for i in range(k):
            src, dst = (self.a, self.b) if i & 1 else (self.b, self.a)
            assert self.lib.hipMemcpyAsync(dst.ptr, src.ptr, C.c_size_t(SCRATCH_BYTES), D2D, C.c_void_p(stream)) == 0

    def hold(self, stream, ms):
        """Keep `stream` busy for at least `ms` (20 .. 160, so that SAFETY x ms stays under the 200 ms ceiling); returns the
        number of copies enqueued."""
        assert HOLD_MIN_MS <= ms <= HOLD_MAX_MS / SAFETY, f"a hold of {ms:.1f} ms is outside [{HOLD_MIN_MS}, {HOLD_MAX_MS / SAFETY}]"
        k = int(math.ceil(SAFETY * ms / self.copy_ms))
        self._copies(stream, k)
        return k

    # -- images
    def stage(self, array):
        """a numpy image in device memory, complete when this returns (hipMalloc + blocking hipMemcpy)"""
        a = np.ascontiguousarray(array)
        buf = DeviceBuffer(self.lib, a.nbytes)
        assert self.lib.hipMemcpy(buf.ptr, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), H2D) == 0
        return buf

    def copy_to_slot(self, stream, slab, index, staged):
        """staged image -> slot `index` of the slab at device address `slab`, asynchronously on `stream`"""
        dst = C.c_void_p(slab + index * staged.nbytes)
        assert self.lib.hipMemcpyAsync(dst, staged.ptr, C.c_size_t(staged.nbytes), D2D, C.c_void_p(stream)) == 0

    def memset_async(self, stream, address, value, nbytes):
        assert self.lib.hipMemsetAsync(C.c_void_p(address), C.c_int(value), C.c_size_t(nbytes), C.c_void_p(stream)) == 0


_holder = None


def holder(ce):
    """one Holder per process: the scratch buffers are 512 MiB and the calibration takes a few milliseconds"""
    global _holder
    if _holder is None:
        _holder = Holder(ce)
    return _holder
