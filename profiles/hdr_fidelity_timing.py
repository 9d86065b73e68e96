"""Kernel timing of the HDR fidelity scores with the library's own per-kernel events (ce_prof_*, solo
times on the context's stream): a linear batch of 6 references and 54 tests of 768x512, ingested from BT.2020 PQ code values
of depth 16, scored by ce_batch_hdr_fidelity at depth 10, 12 and 16 - all 54 pairs in one launch, and one pair alone - and as
the yardstick k_psnr_sse_u16 on a deep batch (16 / 16) of the same shape and pair count.  One warm-up call per phase, then
REPEAT timed calls; the last line printed is the result as JSON.  Per pair and depth the kernel reads 24 bytes a pixel."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

W, H, REFS, PAIRS, REPEAT, WHITE = 768, 512, 6, 54, 20, 203.0
rng = np.random.default_rng(19)
result = {"shape": [W, H], "pairs": PAIRS, "repeat": REPEAT, "mb_per_pair": 24 * W * H / 1e6, "phases": []}
with ce.Context(0) as ctx:
    pq16 = ce.ColourDescription(ce.PRIMARIES_BT2020, ce.TRANSFER_PQ, 16, WHITE)
    refs = [rng.integers(0, 65536, (H, W, 3)).astype(np.uint16) for _ in range(REFS)]
    tests = [np.clip(refs[p % REFS].astype(np.int64) + rng.integers(-300, 301, (H, W, 3)), 0, 65535).astype(np.uint16) for p in range(PAIRS)]
    lin = ctx.batch_linear(W, H, REFS, PAIRS)
    deep = ctx.batch_deep(W, H, REFS, PAIRS, 16, 16)
    for i, r in enumerate(refs):
        lin.set_reference_cicp(i, r, pq16)
        deep.set_reference(i, r)
    for p, t in enumerate(tests):
        lin.set_test_cicp(p, p % REFS, t, pq16)
        deep.set_test(p, p % REFS, t)
    ctx.synchronize()
    ctx.prof_enable(True, serial=True)

    def phase(label, kernel, n_pairs, call, bytes_per_px=24):
        call()  # first use: table upload, code object load
        ctx.synchronize()
        ctx.prof_reset()
        for _ in range(REPEAT):
            call()
        ctx.synchronize()
        launches, ms = ctx.prof_stats()[kernel]
        us = ms * 1e3 / launches
        mb = bytes_per_px * W * H / 1e6 * n_pairs  # MB per us is TB/s
        print(f"{label} [{kernel}]: {launches} launches, {us:.2f} us each, {us / n_pairs:.2f} us a pair, {mb / us:.3f} TB/s of the bytes it must read")
        result["phases"].append({"label": label, "kernel": kernel, "pairs": n_pairs, "launches": launches, "us_per_launch": us,
                                 "us_per_pair": us / n_pairs, "tb_per_s": mb / us})

    for depth in (10, 12, 16):
        phase(f"hdr fidelity depth {depth}, {PAIRS} pairs", f"hdr_fidelity_{depth}", PAIRS, lambda d=depth: lin.hdr_fidelity(PAIRS, d, WHITE))
        phase(f"hdr fidelity depth {depth}, 1 pair", f"hdr_fidelity_{depth}", 1, lambda d=depth: lin.hdr_fidelity(1, d, WHITE))
    psnr = ce.MetricConfig(psnr=True)
    phase(f"yardstick psnr_sse_u16, {PAIRS} pairs (12 B/px: half the bytes)", "psnr_sse_u16", PAIRS, lambda: deep.run(PAIRS, psnr), 12)
    phase("yardstick psnr_sse_u16, 1 pair", "psnr_sse_u16", 1, lambda: deep.run(1, psnr), 12)
    s = lin.hdr_fidelity(2, 16, WHITE)
    print("scores of pairs 0 and 1 at depth 16:", s)
    lin.close()
    deep.close()
print(json.dumps(result))
