"""Tensor ingest on the device (include/ce_metrics.h, section "tensors"): a framework's strided
tensors - numpy arrays on the host, tensors read by address on the device - into the slots of RGB8, deep and linear batches.  The slab
bytes must equal tests/tensor_restatement.py bit for bit for every dtype against every slot kind it may enter, at every
layout; count images in one call must equal count calls; scores and maps must equal those of a batch that was uploaded the
quantised samples; a device tensor must be read behind what the context's stream holds; every refusal is checked by its text."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_hold as SH  # noqa: E402
import tensor_restatement as T  # noqa: E402

pytestmark = pytest.mark.gpu

S = importlib.import_module("codec-eval_amd.session")

# 67 x 5 and the other odd products: w * h * 3 is odd, so the alignment of the RGB8 slots alternates; 64 x 4 and 100 x 76: every
# slot of every kind 16-byte aligned
SHAPES = [(1, 1), (3, 5), (5, 3), (17, 9), (67, 5), (64, 4), (100, 76)]
FLOATS = (T.F16, T.BF16, T.F32)
LAYOUTS = ("chw", "hwc", "rgba", "crop", "gray")
# (batch kind, slot kind of the restatement, depth, the dtypes that may enter)
KINDS = [("rgb8", "u8", 8, (T.U8,) + FLOATS)] + [("deep", "u16", d, ((T.U8,) if d == 8 else ()) + (T.U16,) + FLOATS) for d in (8, 10, 12, 16)] + \
        [("linear", "lin", 0, FLOATS)]
N_SLOTS = 3


def make_batch(ce, ctx, kind, depth, w, h, n=N_SLOTS):
    if kind == "linear":
        return ctx.batch_linear(w, h, n, n)
    return ce.Batch(ctx, w, h, n, n, depths=(depth, depth) if kind == "deep" else None)


def read_slab(ce, address, nbytes):
    """Device bytes -> host after everything queued on the device (the slot writes run on the batch's upload stream)."""
    assert ce.lib().hipDeviceSynchronize() == 0
    out = np.empty(nbytes, np.uint8)
    assert ce.lib().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(address), ctypes.c_size_t(nbytes), 2) == 0
    return out


def backing(rng, dtype, layout, count, w, h, lin):
    """the array a tensor of `layout` is a view of, in its storage dtype (bit patterns for f16 / bf16)"""
    shape = {"chw": (count, 3, h, w), "hwc": (count, h, w, 3), "rgba": (count, h, w, 4), "crop": (count, 3, h + 3, w + 5), "gray": (count, 1, h, w)}[layout]
    return T.sample_elements(rng, dtype, int(np.prod(shape)), lin).reshape(shape)


def view_of(x, layout, count, w, h):
    """the image tensor inside its backing array or tensor, and the names of its axes"""
    if layout in ("hwc", "rgba"):
        return x, "NHWC"
    if layout == "crop":
        return x[:, :, 1:1 + h, 2:2 + w], "NCHW"
    if layout == "gray":
        return np.broadcast_to(x, (count, 3, h, w)), "NCHW"
    return x, "NCHW"


def elements(back, layout, count, w, h):
    """[count][h][w][3] storage elements of the view"""
    v, names = view_of(back, layout, count, w, h)
    return (v if names == "NHWC" else np.transpose(v, (0, 2, 3, 1)))[..., :3]


def stage(ce, array):
    """a numpy array in device memory, complete when this returns (hipMalloc + blocking hipMemcpy through the library's runtime)"""
    a = np.ascontiguousarray(array)
    buf = SH.DeviceBuffer(ce.lib(), max(a.nbytes, 1))
    assert ce.lib().hipMemcpy(buf.ptr, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes), SH.H2D) == 0
    return buf


class DeviceTensor:
    """What TensorImage.from_array reads of a framework's device tensor - data_ptr(), stride() in elements, shape, a dtype known
    by its name, is_cuda - over a device copy of a numpy view's backing array.  (A real torch tensor is read the same way,
    tests/test_tensor_ingest_cpu.py; this one is allocated by the library's own HIP runtime, which every machine that runs
    the suite has.)"""
    is_cuda = True
    NAMES = {T.U8: "torch.uint8", T.U16: "torch.uint16", T.F16: "torch.float16", T.BF16: "torch.bfloat16", T.F32: "torch.float32"}

    def __init__(self, ce, back, view, dtype):
        self.buf = stage(ce, back)
        self.shape, self.dtype = tuple(view.shape), self.NAMES[dtype]
        self._stride = tuple(s // view.itemsize for s in view.strides)
        self._ptr = self.buf.address + view.__array_interface__["data"][0] - back.__array_interface__["data"][0]

    def data_ptr(self):
        return self._ptr

    def stride(self):
        return self._stride


def as_tensor(ce, back, dtype, layout, count, w, h, device, quantise):
    """the TensorImage of the view: numpy on the host (bf16 and f16 as their bit patterns), a device tensor read by address"""
    if not device:
        v, names = view_of(back.view(np.float16) if dtype == T.F16 and count % 2 else back, layout, count, w, h)  # either form of f16
        return ce.TensorImage.from_array(v, names, quantise, dtype=dtype if v.dtype == np.uint16 else None)
    v, names = view_of(back, layout, count, w, h)
    img = ce.TensorImage.from_array(DeviceTensor(ce, back, v, dtype), names, quantise)
    assert img.memory == ce.MEM_DEVICE and img.dtype == dtype
    return img


def slot_dtype(slot):
    return {"u8": np.uint8, "u16": np.uint16, "lin": np.uint32}[slot]


def want_slot(el, dtype, slot, depth, rule):
    out = T.to_slot(el, dtype, slot, depth, rule)
    return out.view(np.uint32) if slot == "lin" else out


@pytest.mark.parametrize("w,h", SHAPES)
def test_slab_bytes_equal_the_restatement(ce, gpu_ctx, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    n_calls = 0
    for kind, slot, depth, dtypes in KINDS:
        batch = make_batch(ce, gpu_ctx, kind, depth, w, h)
        dt = slot_dtype(slot)
        per = w * h * 3
        try:
            want = {side: np.zeros((N_SLOTS, per), dt) for side in ("ref", "test")}
            for side in want:  # known bytes in every slot first, so that a neighbour that changes shows
                filler = T.sample_elements(rng, T.F32 if slot == "lin" else T.U8, N_SLOTS * per).reshape(N_SLOTS, per)
                for k in range(N_SLOTS):
                    px = filler[k].astype(np.float32 if slot == "lin" else np.uint16 if slot == "u16" else np.uint8)
                    if slot == "lin":
                        px = T.linear(px, T.F32)
                    batch.set_reference(k, px) if side == "ref" else batch.set_test(k, k, px)
                    want[side][k] = px.view(dt)
            for dtype in dtypes:
                for rule in ((T.NEAREST_EVEN, T.TRUNCATE) if dtype in FLOATS and slot != "lin" else (T.NEAREST_EVEN,)):
                    for layout in LAYOUTS:
                        for device in (False, True):
                            k, side = n_calls % N_SLOTS, ("ref", "test")[(n_calls // N_SLOTS) % 2]
                            n_calls += 1
                            back = backing(rng, dtype, layout, 1, w, h, slot == "lin")
                            img = as_tensor(ce, back, dtype, layout, 1, w, h, device, rule)
                            if side == "ref":
                                batch.set_reference_tensor(k, img)
                            else:
                                batch.set_test_tensor(k, [(k + 1) % N_SLOTS], img)
                            want[side][k] = want_slot(elements(back, layout, 1, w, h), dtype, slot, depth, rule).reshape(-1)
                            address = batch.reference_slab if side == "ref" else batch.test_slab
                            got = read_slab(ce, address, want[side].nbytes).view(dt).reshape(N_SLOTS, per)
                            assert np.array_equal(got, want[side]), (kind, depth, dtype, rule, layout, device, side, k)
        finally:
            batch.close()
    assert n_calls >= 150


@pytest.mark.parametrize("dtype", (T.U8, T.U16) + FLOATS)
def test_a_full_size_image_and_the_leaves(ce, gpu_ctx, dtype):
    """768 x 512, where a launch is hundreds of blocks and the fast paths run; the leaves equal the batch route"""
    w, h = 768, 512
    rng = np.random.default_rng(dtype)
    for kind, slot, depth, dtypes in KINDS:
        if dtype not in dtypes or depth not in (0, 8, 10):
            continue
        batch = make_batch(ce, gpu_ctx, kind, depth, w, h, 1)
        try:
            for layout, device in (("chw", True), ("hwc", True), ("rgba", False), ("crop", True)):
                back = backing(rng, dtype, layout, 1, w, h, slot == "lin")
                img = as_tensor(ce, back, dtype, layout, 1, w, h, device, T.NEAREST_EVEN)
                want = want_slot(elements(back, layout, 1, w, h), dtype, slot, depth, T.NEAREST_EVEN)[0]
                batch.set_test_tensor(0, [0], img)
                got = read_slab(ce, batch.test_slab, want.nbytes).view(want.dtype).reshape(want.shape)
                assert np.array_equal(got, want), (kind, depth, layout, device)
                leaf = gpu_ctx.tensor_to_linear(img) if slot == "lin" else gpu_ctx.tensor_to_rgb8(img) if slot == "u8" else gpu_ctx.tensor_to_rgb16(img, depth)
                assert np.array_equal(leaf.view(want.dtype), want), ("leaf", kind, depth, layout, device)
        finally:
            batch.close()


@pytest.mark.parametrize("w,h", [(67, 5), (100, 76)])
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_count_images_in_one_call_equal_as_many_calls(ce, gpu_ctx, w, h, device):
    rng = np.random.default_rng(9)
    for kind, slot, depth, dtypes in (KINDS[0], KINDS[2], KINDS[5]):
        one, each = make_batch(ce, gpu_ctx, kind, depth, w, h), make_batch(ce, gpu_ctx, kind, depth, w, h)
        try:
            for dtype in (dtypes[0], T.BF16, T.F32):
                for layout in LAYOUTS:
                    back = backing(rng, dtype, layout, 3, w, h, slot == "lin")
                    # device tensors stay alive until their slots have been read back
                    keep = [as_tensor(ce, back, dtype, layout, 3, w, h, device, T.TRUNCATE if slot == "u8" and dtype != T.U8 else 0),
                            as_tensor(ce, back, dtype, layout, 3, w, h, device, 0)]
                    one.set_reference_tensor(0, keep[0])
                    one.set_test_tensor(0, [2, 1, 0], keep[1])
                    assert one._pair_ref == [2, 1, 0]
                    for n in range(3):
                        img = as_tensor(ce, np.ascontiguousarray(back[n:n + 1]), dtype, layout, 1, w, h, device, 0)
                        keep.append(img)
                        each.set_test_tensor(n, [0], img)
                        leaf = gpu_ctx.tensor_to_linear(img) if slot == "lin" else gpu_ctx.tensor_to_rgb8(img) if slot == "u8" else gpu_ctx.tensor_to_rgb16(img, depth)
                        want = want_slot(elements(back, layout, 3, w, h)[n], dtype, slot, depth, 0)
                        assert np.array_equal(leaf.view(want.dtype), want)
                    nbytes = 3 * w * h * 3 * slot_dtype(slot)().itemsize
                    a, b = read_slab(ce, one.test_slab, nbytes), read_slab(ce, each.test_slab, nbytes)
                    assert np.array_equal(a, b), (kind, dtype, layout)
                    assert np.array_equal(a.view(slot_dtype(slot)).reshape(3, h, w, 3), want_slot(elements(back, layout, 3, w, h), dtype, slot, depth, 0))
        finally:
            one.close()
            each.close()


def scores_tuple(s):
    return (s.status, s.valid, s.dssim, s.ssimulacra2, s.butteraugli, s.psnr)


def test_scores_and_diffmap_equal_a_batch_uploaded_the_quantised_samples(ce, gpu_ctx, workloads):
    w, h = 100, 76
    ref8 = workloads.make_reference(w, h, 3).reshape(h, w, 3)
    rng = np.random.default_rng(4)
    x = np.clip(ref8.astype(np.float32) / 255.0 + rng.normal(0, 0.02, (h, w, 3)).astype(np.float32), -0.05, 1.05).astype(np.float32)  # a "decoded" HWC float image
    chw = np.ascontiguousarray(x.transpose(2, 0, 1))
    dev = DeviceTensor(ce, chw, chw, T.F32)  # CHW on the device, as a model returns it
    cfg = ce.MetricConfig.all()
    for kind, depth in (("rgb8", 8), ("deep", 10), ("linear", 0)):
        got_b, want_b = make_batch(ce, gpu_ctx, kind, depth, w, h, 2), make_batch(ce, gpu_ctx, kind, depth, w, h, 2)
        try:
            if kind == "linear":
                lin = ce.srgb_table(8, 0)[ref8].astype(np.float32)
                quant = [T.linear(x, T.F32)] * 2
                refs = lin
            else:
                quant = [ce.quantise_tensor(x, depth, rule) for rule in (ce.QUANT_NEAREST_EVEN, ce.QUANT_TRUNCATE)]
                refs = ref8 if kind == "rgb8" else (ref8.astype(np.uint32) * 1023 // 255).astype(np.uint16)
            for b in (got_b, want_b):
                b.set_reference(0, refs)
            got_b.set_test_tensor(0, [0], ce.TensorImage.from_array(dev, "CHW"))
            got_b.set_test_tensor(1, [0], ce.TensorImage.from_array(x, "HWC", quantise=ce.QUANT_NEAREST_EVEN if kind == "linear" else ce.QUANT_TRUNCATE))
            if kind == "rgb8":
                want_b.set_test(0, 0, quant[0])
                want_b.set_test(1, 0, quant[1])
            else:
                want_b.set_test_fmt(0, 0, quant[0], ce.PIXEL_RGB_F32 if kind == "linear" else ce.PIXEL_RGB16)
                want_b.set_test_fmt(1, 0, quant[1], ce.PIXEL_RGB_F32 if kind == "linear" else ce.PIXEL_RGB16)
            got = got_b.run(2, cfg, butteraugli_diffmap=True)
            want = want_b.run(2, cfg, butteraugli_diffmap=True)
            assert [scores_tuple(s) for s in got] == [scores_tuple(s) for s in want], kind
            assert all(s.status == 0 for s in got)
            assert np.array_equal(got_b.butteraugli_diffmaps(0, 2), want_b.butteraugli_diffmaps(0, 2)), kind
        finally:
            got_b.close()
            want_b.close()


def test_the_rounding_rule_is_applied_and_matters(ce, gpu_ctx):
    w, h = 100, 76
    rng = np.random.default_rng(6)
    x = rng.uniform(0, 1, (3, h, w)).astype(np.float32)
    batch = ce.Batch(gpu_ctx, w, h, 1, 2)
    try:
        batch.set_reference_tensor(0, ce.TensorImage.from_array(x, "CHW", quantise=ce.QUANT_NEAREST_EVEN))
        batch.set_test_tensor(0, [0], ce.TensorImage.from_array(x, "CHW", quantise=ce.QUANT_NEAREST_EVEN))
        batch.set_test_tensor(1, [0], ce.TensorImage.from_array(x, "CHW", quantise=ce.QUANT_TRUNCATE))
        same, other = batch.run(2, ce.MetricConfig.all())
        assert same.status == 0 and other.status == 0
        assert same.dssim == 0.0 and same.butteraugli == 0.0 and same.ssimulacra2 == 100.0
        assert np.isfinite(other.psnr) and other.butteraugli > 0.0 and other.ssimulacra2 < 100.0 and other.dssim > 0.0
    finally:
        batch.close()


@pytest.fixture(scope="module")
def H(ce, gpu_ctx):
    return SH.holder(ce)


def stream_rig(ce, workloads, w, h):
    """a reference, three float CHW test images A, B, C and the bytes each quantises to"""
    ref = workloads.make_reference(w, h, 11)
    imgs = []
    for seed, q in ((12, 30), (13, 60), (14, 85)):
        t8 = workloads.distort(workloads.make_reference(w, h, 11), q).reshape(h, w, 3)
        imgs.append(np.ascontiguousarray((t8.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)))
    return ref, imgs


def test_a_device_tensor_is_read_behind_the_contexts_stream(ce, gpu_ctx, workloads, H):
    """The context's stream is held; behind the hold a copy on that stream replaces the tensor's contents with image B; then
    set_test_tensor with no host synchronisation and a run: the scores are B's."""
    w, h = 100, 76
    ref, (A, B, _) = stream_rig(ce, workloads, w, h)
    cfg = ce.MetricConfig.all()
    tensor, staged_b = H.stage(A), H.stage(B)
    img = ce.TensorImage(tensor.address, (3 * h * w, h * w, w, 1), 1, h, w, ce.DTYPE_F32, ce.MEM_DEVICE, keep=tensor)
    batch, plain = ce.Batch(gpu_ctx, w, h, 1, 1), ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        want = {}
        for name, x in (("A", A), ("B", B)):
            plain.set_reference(0, ref)
            plain.set_test(0, 0, ce.quantise_tensor(x.transpose(1, 2, 0), 8))
            want[name] = scores_tuple(plain.run(1, cfg)[0])
        assert want["A"] != want["B"]
        batch.set_reference(0, ref)
        batch.set_test_tensor(0, [0], img)
        assert scores_tuple(batch.run(1, cfg)[0]) == want["A"]  # warms the path
        gpu_ctx.synchronize()
        S_ = gpu_ctx.stream
        H.hold(S_, SH.HOLD_MIN_MS)
        assert ce.lib().hipMemcpyAsync(tensor.ptr, staged_b.ptr, ctypes.c_size_t(B.nbytes), SH.D2D, ctypes.c_void_p(S_)) == 0
        batch.set_test_tensor(0, [0], img)
        busy = H.busy(S_)
        batch.launch(1, cfg)
        got = scores_tuple(batch.collect(1)[0])
        print(f"[tensor stream-order] stream busy when the setter returned: {busy}")
        assert busy, "hold too short: the stream was idle when the setter returned (or the setter waits for it)"
        assert got == want["B"]
    finally:
        gpu_ctx.synchronize()
        batch.close()
        plain.close()


def test_a_setter_between_launch_and_collect_does_not_disturb_the_launch(ce, gpu_ctx, workloads, H):
    w, h = 100, 76
    ref, (A, B, Cimg) = stream_rig(ce, workloads, w, h)
    cfg = ce.MetricConfig.all()
    tensors = {name: H.stage(x) for name, x in (("B", B), ("C", Cimg))}
    image = lambda name: ce.TensorImage(tensors[name].address, (3 * h * w, h * w, w, 1), 1, h, w, ce.DTYPE_F32, ce.MEM_DEVICE, keep=tensors[name])
    batch = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        batch.set_reference(0, ref)
        want = {}
        for name in ("C", "B"):
            batch.set_test_tensor(0, [0], image(name))
            want[name] = scores_tuple(batch.run(1, cfg)[0])
        assert want["B"] != want["C"]  # the batch now holds B
        gpu_ctx.synchronize()
        H.hold(gpu_ctx.stream, SH.HOLD_MIN_MS)
        batch.launch(1, cfg)
        busy = H.busy(gpu_ctx.stream)
        batch.set_test_tensor(0, [0], image("C"))
        batch.set_test_tensor(0, [0], ce.TensorImage.from_array(Cimg, "CHW"))  # and the host route
        first = scores_tuple(batch.collect(1)[0])
        second = scores_tuple(batch.run(1, cfg)[0])
        assert busy, "hold too short: the stream was idle when the launch returned"
        assert first == want["B"] and second == want["C"]
    finally:
        gpu_ctx.synchronize()
        batch.close()


def test_session_rows_equal_those_of_the_quantised_bytes(ce, gpu_ctx, workloads, tmp_path):
    w, h = 96, 80
    src = workloads.make_reference(w, h, 7)

    def codec(as_tensor_image):
        def encode(image, request):
            return np.array([int(request.quality)], np.uint32).tobytes() + image.to_rgb8_vec().tobytes()

        def decode(blob):
            q = int(np.frombuffer(blob[:4], np.uint32)[0])
            rgb = np.frombuffer(blob[4:], np.uint8).reshape(h, w, 3)
            x = (rgb.astype(np.float32) / np.float32(255.0) * np.float32(q / 100.0) + np.float32(0.013)).astype(np.float32)  # a model's float output
            chw = np.ascontiguousarray(x.transpose(2, 0, 1))
            if as_tensor_image:
                return S.ImageData.tensor(DeviceTensor(ce, chw, chw, T.F32) if q != 75 else chw, "CHW")  # device tensors, and one host array
            return S.ImageData.rgb(ce.quantise_tensor(x, 8), w, h)
        return encode, decode

    rows = []
    for as_tensor_image in (True, False):
        cfg = S.EvalConfig.builder().report_dir(tmp_path / f"rep{int(as_tensor_image)}").metrics(ce.MetricConfig.all()).quality_levels([50, 75, 95]).build()
        ses = S.EvalSession(cfg, ctx=gpu_ctx)
        ses.add_codec_with_decode("toy", "1.0", *codec(as_tensor_image))
        source = S.ImageData.tensor(src.reshape(h, w, 3), "HWC") if as_tensor_image else S.ImageData.rgb(src, w, h)
        rep = ses.evaluate_image("pattern.png", source)
        rows.append([(r.quality, r.psnr, r.ssimulacra2, r.dssim, r.butteraugli, r.perception, r.file_size) for r in rep.results])
    assert rows[0] == rows[1] and len(rows[0]) == 3 and all(r[1] is not None for r in rows[0])
    x = np.linspace(-0.1, 1.1, w * h * 3, dtype=np.float32).reshape(3, h, w)
    assert np.array_equal(S.ImageData.tensor(x, "CHW").to_rgb8_vec(), ce.quantise_tensor(x.transpose(1, 2, 0), 8).reshape(-1))


def test_refusals(ce, gpu_ctx):
    w, h = 17, 9
    L = ce.lib()
    x = np.full((3, h, w), 0.5, np.float32)
    u8 = np.full((3, h, w), 7, np.uint8)
    u16 = np.full((3, h, w), 700, np.uint16)
    rgb8, deep10, linear = ce.Batch(gpu_ctx, w, h, 2, 2), ce.Batch(gpu_ctx, w, h, 2, 2, depths=(10, 10)), gpu_ctx.batch_linear(w, h, 2, 2)

    def refused(batch, image, text, count=None, first=0, refs=None, test=False):
        c = image._c() if image is not None else None
        n = count if count is not None else image.count if image is not None else 1
        if test:
            r = None if refs == "null" else np.ascontiguousarray([0] * max(n, 1) if refs is None else refs, dtype=np.uint32)
            rc = L.ce_batch_set_test_tensor(batch._h, first, None if r is None else r.ctypes.data, n, ctypes.byref(c) if c is not None else None)
        else:
            rc = L.ce_batch_set_reference_tensor(batch._h, first, n, ctypes.byref(c) if c is not None else None)
        assert rc == ce.CE_ERR_INVALID_ARG and text in gpu_ctx._err(), (rc, gpu_ctx._err(), text)

    def edited(image, **kw):
        t = ce.TensorImage(image.data, image.strides, image.count, image.height, image.width, image.dtype, image.memory, image.quantise, keep=image.keep)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    try:
        good = ce.TensorImage.from_array(x, "CHW")
        refused(rgb8, None, "tensor ingest: null pointer")
        refused(rgb8, edited(good, data=0), "tensor ingest: null pointer")
        refused(rgb8, good, "tensor ingest: null pointer", refs="null", test=True)
        refused(rgb8, edited(good, dtype=5), "unknown dtype 5")
        refused(rgb8, edited(good, dtype=-1), "unknown dtype -1")
        refused(rgb8, edited(good, memory=2), "unknown memory kind 2")
        refused(rgb8, edited(good, quantise=2), "unknown quantise rule 2")
        refused(rgb8, ce.TensorImage.from_array(u8, "CHW", quantise=ce.QUANT_TRUNCATE), "quantise is for float dtypes into integer slots")
        refused(linear, ce.TensorImage.from_array(x, "CHW", quantise=ce.QUANT_TRUNCATE), "quantise is for float dtypes into integer slots")
        refused(rgb8, edited(good, strides=(0, -(h * w), w, 1)), "negative stride")
        refused(rgb8, ce.TensorImage.from_array(x[:, :, ::-1], "CHW"), "negative stride")
        refused(rgb8, edited(good, strides=(0, h * w, w, 0)), "stride_x and stride_y must be at least 1")
        refused(rgb8, edited(good, strides=(0, h * w, 0, 1)), "stride_x and stride_y must be at least 1")
        refused(rgb8, edited(good, data=good.data + 2), "not aligned to its 4-byte elements")
        refused(deep10, edited(ce.TensorImage.from_array(u16, "CHW"), data=u16.ctypes.data + 1), "not aligned to its 2-byte elements")
        refused(rgb8, edited(good, strides=(0, h * w, 1 << 62, 1)), "extent overflows size_t")
        refused(rgb8, edited(good, strides=(1 << 62, h * w, w, 1), count=2), "extent overflows size_t")
        refused(deep10, ce.TensorImage.from_array(u8, "CHW"), "an 8-bit tensor needs a side of depth 8, this one has 10")
        refused(rgb8, ce.TensorImage.from_array(u16, "CHW"), "CE_DTYPE_U16 needs a deep batch")
        refused(linear, ce.TensorImage.from_array(u8, "CHW"), "a linear batch takes float tensors")
        refused(linear, ce.TensorImage.from_array(u16, "CHW"), "a linear batch takes float tensors")
        refused(rgb8, good, "count must be 1 to 65535, got 0", count=0)
        refused(rgb8, edited(good, strides=(0, h * w, w, 1)), "tensor ingest: reference slots [1, 4) outside the 2 slots", count=3, first=1)
        refused(rgb8, edited(good, strides=(0, h * w, w, 1)), "tensor ingest: test slots [2, 3) outside the 2 slots", count=1, first=2, test=True)
        refused(rgb8, edited(good, strides=(0, h * w, w, 1)), "tensor ingest: test slots [0, 3) outside the 2 slots", count=3, test=True)
        refused(rgb8, good, "tensor ingest: ref index 2 out of range", refs=[2], test=True)
        refused(rgb8, edited(good, strides=(0, h * w, w, 2)), "make it contiguous or pass device memory")
        refused(rgb8, edited(good, strides=(0, 2, w * 3, 3)), "make it contiguous or pass device memory")
        refused(rgb8, edited(good, strides=(0, 1, w * 5, 5)), "make it contiguous or pass device memory")
        with pytest.raises(ValueError):
            rgb8.set_reference_tensor(0, ce.TensorImage.from_array(np.zeros((3, h, w + 1), np.float32), "CHW"))
        # the leaves: the same refusals, a bad depth and a wrong length
        c = good._c()
        out = np.empty(w * h * 3, np.uint16)
        assert L.ce_tensor_to_rgb16(gpu_ctx._h, ctypes.byref(c), w, h, 9, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
        assert "output depth must be 8, 10, 12 or 16" in gpu_ctx._err()
        assert L.ce_tensor_to_rgb8(gpu_ctx._h, ctypes.byref(c), w, h, out.ctypes.data, 5) == ce.CE_ERR_BAD_LENGTH
        assert L.ce_tensor_to_rgb8(gpu_ctx._h, None, w, h, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG and "null pointer" in gpu_ctx._err()
        assert L.ce_tensor_to_rgb8(gpu_ctx._h, ctypes.byref(c), 0, h, out.ctypes.data, 0) == ce.CE_ERR_INVALID_ARG and "empty image" in gpu_ctx._err()
        assert L.ce_tensor_to_linear(gpu_ctx._h, ctypes.byref(ce.TensorImage.from_array(u8, "CHW")._c()), w, h, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
        # every batch is still usable
        for batch, slot, depth in ((rgb8, "u8", 8), (deep10, "u16", 10), (linear, "lin", 0)):
            batch.set_reference_tensor(0, good)
            batch.set_test_tensor(0, [0], good)
            batch.set_test_tensor(1, [0], good)
            want = want_slot(x.transpose(1, 2, 0), T.F32, slot, depth, 0)
            got = read_slab(ce, batch.test_slab, 2 * want.nbytes).view(want.dtype).reshape(2, h, w, 3)[1]
            assert np.array_equal(got, want)
            assert batch.run(2, ce.MetricConfig(ssimulacra2=True))[1].ssimulacra2 == 100.0
    finally:
        for b in (rgb8, deep10, linear):
            b.close()
