"""Kernel timing of the Delta E ITP maps with the library's own per-kernel events (ce_prof_*, solo times
on the context's stream): the batch of profiles/hdr_fidelity_timing.py - 6 references and 54 tests of 768x512, ingested from
BT.2020 PQ code values of depth 16 - through ce_batch_delta_e_itp_map at depth 10, 12 and 16: the full map (block 1), the cell
maxima of block 8 and the counts alone, each with four thresholds, and as the yardstick hdr_fidelity_<depth> on the same batch
in the same run.  One warm-up call per phase, then REPEAT timed calls; beside the kernel's time the host clock's time per Python
call, which at block 1 carries the copy of 54 x 768 x 512 x 4 bytes to pageable memory.  The last line printed is the result as
JSON."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

W, H, REFS, PAIRS, REPEAT, WHITE = 768, 512, 6, 54, 20, 203.0
THR = [0, ce.DELTA_E_ITP_Q20, 5 * ce.DELTA_E_ITP_Q20, (1 << 32) - 1]
rng = np.random.default_rng(19)
result = {"shape": [W, H], "pairs": PAIRS, "repeat": REPEAT, "map_mb": 4 * W * H * PAIRS / 1e6, "phases": []}
with ce.Context(0) as ctx:
    pq16 = ce.ColourDescription(ce.PRIMARIES_BT2020, ce.TRANSFER_PQ, 16, WHITE)
    refs = [rng.integers(0, 65536, (H, W, 3)).astype(np.uint16) for _ in range(REFS)]
    tests = [np.clip(refs[p % REFS].astype(np.int64) + rng.integers(-300, 301, (H, W, 3)), 0, 65535).astype(np.uint16) for p in range(PAIRS)]
    lin = ctx.batch_linear(W, H, REFS, PAIRS)
    for i, r in enumerate(refs):
        lin.set_reference_cicp(i, r, pq16)
    for p, t in enumerate(tests):
        lin.set_test_cicp(p, p % REFS, t, pq16)
    ctx.synchronize()
    ctx.prof_enable(True, serial=True)

    def phase(label, kernel, call):
        call()  # first use: table upload, code object load, the map buffer
        ctx.synchronize()
        ctx.prof_reset()
        t0 = time.perf_counter()
        for _ in range(REPEAT):
            call()
        ctx.synchronize()
        call_ms = (time.perf_counter() - t0) * 1e3 / REPEAT
        launches, ms = ctx.prof_stats()[kernel]
        us = ms * 1e3 / launches
        print(f"{label} [{kernel}]: {launches} launches, {us:.2f} us each, {us / PAIRS:.2f} us a pair; {call_ms:.3f} ms a Python call")
        result["phases"].append({"label": label, "kernel": kernel, "launches": launches, "us_per_launch": us, "us_per_pair": us / PAIRS,
                                 "ms_per_call": call_ms})
        return us

    for depth in (10, 12, 16):
        k = f"delta_e_itp_map_{depth}"
        base = phase(f"yardstick hdr fidelity depth {depth}", f"hdr_fidelity_{depth}", lambda d=depth: lin.hdr_fidelity(PAIRS, d, WHITE))
        full = phase(f"map depth {depth} block 1", k, lambda d=depth: lin.delta_e_itp_maps(0, PAIRS, d, WHITE, 1, THR))
        cell = phase(f"map depth {depth} block 8", k, lambda d=depth: lin.delta_e_itp_maps(0, PAIRS, d, WHITE, 8, THR))
        only = phase(f"map depth {depth} counts only", k, lambda d=depth: lin.delta_e_itp_maps(0, PAIRS, d, WHITE, 1, THR, maps=False))
        print(f"depth {depth}: block 1 / yardstick {full / base:.3f}, block 8 / yardstick {cell / base:.3f}, counts only / yardstick {only / base:.3f}")
        result["phases"].append({"label": f"ratios depth {depth}", "block1": full / base, "block8": cell / base, "counts_only": only / base})
    maps, over = lin.delta_e_itp_maps(0, 2, 16, WHITE, 1, THR)
    s = lin.hdr_fidelity(2, 16, WHITE)
    print("pairs 0 and 1 at depth 16: over", over.tolist(), "map sums", [int(m.astype(np.uint64).sum()) for m in maps], "itp_sum_q20",
          [x.itp_sum_q20 for x in s])
    lin.close()
print(json.dumps(result))
