"""Generator of yuv_pillow.npz: what libjpeg-turbo (through Pillow) decodes from small JPEG files, as the fixture that
pins the Y'CbCr ingest definition (tests/yuv_restatement.py) on hosts without Pillow.

    python tests/golden/make_yuv_pillow.py            # rewrites tests/golden/yuv_pillow.npz

Per case `<sub>_<w>x<h>` (sub = 444, 422, 420: the file's chroma subsampling):
    <case>_rgb    (h, w, 3) u8   the file opened normally: libjpeg's upsampling + jdcolor.c
    <case>_ycc    (h, w, 3) u8   opened with draft('YCbCr', (w, h)): the upsampled Y'CbCr, before the colour conversion
    <case>_half   (h', w', 3) u8 4:2:0 only, draft('YCbCr', (w // 2, h // 2)): at scale 1/2 libjpeg gives chroma its full
                                 IDCT and no upsampling, so channels 1 and 2 are the file's raw subsampled chroma planes when
                                 (h', w') = (ceil(h / 2), ceil(w / 2)); luma is a scaled IDCT and is not used
`pillow` holds the Pillow version that wrote the file.
"""
import io
import os

import numpy as np
import PIL
from PIL import Image

SHAPES = [(48, 32), (37, 21), (16, 16), (9, 301), (100, 76)]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def picture(w, h, seed):
    """a smooth gradient with noise and a few hard colour edges, so chroma differs between neighbouring samples"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), 255.0 - (xx + yy) * 255.0 / max(w + h - 2, 1)], -1)
    img += rng.normal(0, 24, img.shape)
    img[h // 3: h // 3 + max(h // 5, 1), w // 4: w // 4 + max(w // 3, 1)] = rng.integers(0, 256, 3)
    img[:: 7, :: 5] = rng.integers(0, 256, (len(range(0, h, 7)), len(range(0, w, 5)), 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    out = {"pillow": np.array(PIL.__version__)}
    for sub, code in SUBSAMPLING.items():
        for i, (w, h) in enumerate(SHAPES):
            buf = io.BytesIO()
            Image.fromarray(picture(w, h, 100 * code + i)).save(buf, "JPEG", quality=92, subsampling=code)
            data = buf.getvalue()
            case = f"{sub}_{w}x{h}"
            out[case + "_rgb"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            im = Image.open(io.BytesIO(data))
            im.draft("YCbCr", (w, h))
            assert im.mode == "YCbCr" and im.size == (w, h)
            out[case + "_ycc"] = np.asarray(im)
            if sub == "420":
                im = Image.open(io.BytesIO(data))
                im.draft("YCbCr", (w // 2, h // 2))
                out[case + "_half"] = np.asarray(im)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "yuv_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if k.endswith("_half")})


if __name__ == "__main__":
    main()
