"""Writes tests/golden/resample_pillow.npz: small inputs and what Pillow's Image.resize returns for them, for the four
filters x the eight ratios of tests/resample_restatement.py on three shapes.  Run once where PIL is installed:
    python tests/golden/make_resample_golden.py
Keys: in_<i> = (h, w, 3) input; out_<i>_<num>_<den>_<filter> = Pillow's output at scaled(w), scaled(h)."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_restatement as R  # noqa: E402

INPUTS = ((100, 76, "pattern"), (33, 25, "noise"), (9, 31, "noise"))
PIL_FILTER = {R.BOX: Image.BOX, R.BILINEAR: Image.BILINEAR, R.BICUBIC: Image.BICUBIC, R.LANCZOS3: Image.LANCZOS}

if __name__ == "__main__":
    out = {}
    for i, (w, h, kind) in enumerate(INPUTS):
        img = R.content(w, h, kind)
        out[f"in_{i}"] = img
        for num, den in R.CASE_RATIOS:
            for f in R.FILTERS:
                size = (R.scaled(w, num, den), R.scaled(h, num, den))
                out[f"out_{i}_{num}_{den}_{f}"] = np.asarray(Image.fromarray(img).resize(size, PIL_FILTER[f]))
    path = os.path.join(HERE, "resample_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays, Pillow", Image.__version__)
