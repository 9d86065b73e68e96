"""Writes tests/golden/resample_linear_pillow.npz: small float inputs and what Pillow's Image.resize returns for them as
mode "F" images, for box, bilinear and bicubic (their weights use no libm call, so the outputs are the same on any host;
Lanczos is pinned against a live Pillow in test_resample_linear_cpu.py) x the eight ratios of tests/resample_restatement.py
on three shapes.  Run once where PIL is installed:
    python tests/golden/make_resample_linear_golden.py
Keys: in_<i> = (h, w, 3) float32 input; out_<i>_<num>_<den>_<filter> = Pillow's output at scaled(w), scaled(h)."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_linear_restatement as RL  # noqa: E402

INPUTS = ((16, 12), (11, 9), (5, 13))
RECORDED_FILTERS = (RL.BOX, RL.BILINEAR, RL.BICUBIC)
PIL_FILTER = {RL.BOX: Image.BOX, RL.BILINEAR: Image.BILINEAR, RL.BICUBIC: Image.BICUBIC, RL.LANCZOS3: Image.LANCZOS}


def pillow_resize(img, out_w, out_h, filt):
    """(h, w, 3) float32 through Image.resize, channel by channel (a 2-D float32 array becomes a mode "F" image)."""
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(img[..., c])).resize((out_w, out_h), PIL_FILTER[filt]))
                     for c in range(3)], axis=2)


if __name__ == "__main__":
    out = {}
    for i, (w, h) in enumerate(INPUTS):
        img = RL.content(w, h, seed=i)
        out[f"in_{i}"] = img
        for num, den in RL.CASE_RATIOS:
            for f in RECORDED_FILTERS:
                out[f"out_{i}_{num}_{den}_{f}"] = pillow_resize(img, RL.scaled(w, num, den), RL.scaled(h, num, den), f)
    path = os.path.join(HERE, "resample_linear_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays, Pillow", Image.__version__)
