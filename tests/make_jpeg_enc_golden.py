"""Makes tests/golden/jpeg_enc: the inputs of the encoder's tests and the streams Pillow (libjpeg-turbo's default compressor) writes for them,

    Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s, restart_marker_blocks=r)

with ``optimize`` off and no dpi / exif / icc.  Run once on the build machine:

    python -m tests.make_jpeg_enc_golden

Every fixture is one .npz with ``pixels`` (the input, uint8: [h, w, 3] R G B, or [h, w] for a grey case), ``jpg`` (Pillow's stream), ``decoded``
(what Pillow decodes from that stream: the round trip; stored for the 8x9 and 33x50 cases) and ``params`` (quality, restart interval in MCUs as the stream's DRI states it).  The
tests read the committed files; tests/test_jpeg_enc_host.py encodes again where Pillow is importable and compares."""
import io
import os

import numpy as np

from tests.make_jpeg_golden import MODES, SUBSAMPLING, image

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc")
SIZES = ((1, 1), (8, 9), (16, 16), (17, 23), (33, 50), (40, 31))   # h x w
MCU = {"grey": (8, 8), "444": (8, 8), "422": (8, 16), "420": (16, 16)}   # h x w


def cases():
    """-> {name: (h, w, mode, quality, restart interval in MCUs)} in a fixed order"""
    out = {}
    for (h, w) in SIZES:
        for mode in MODES:
            for q in (50, 95):
                out[f"{h}x{w}_{mode}_q{q}"] = (h, w, mode, q, 0)
    for q in (10, 75, 100):
        out[f"33x50_420_q{q}"] = (33, 50, "420", q, 0)
    out["33x50_420_rst2"] = (33, 50, "420", 75, 2)
    out["33x50_420_rstrow"] = (33, 50, "420", 75, -(-50 // 16))
    out["75x100_444_rst1"] = (75, 100, "444", 50, 1)                # 130 intervals
    return out


def pixels(h, w, mode):
    a = image(h, w)
    return np.ascontiguousarray(a[..., 1]) if mode == "grey" else a


def pillow_encode(a, mode, quality, restart):
    from PIL import Image
    b = io.BytesIO()
    kw = dict(restart_marker_blocks=restart) if restart else {}
    if mode != "grey":
        kw["subsampling"] = SUBSAMPLING[mode]
    Image.fromarray(a).save(b, "JPEG", quality=quality, **kw)
    return b.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def load_all():
    """the committed fixtures (no Pillow needed) -> {name: dict(pixels, jpg bytes, decoded, mode, quality, restart)}"""
    out = {}
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            z = np.load(os.path.join(HERE, f))
            name = f[:-4]
            out[name] = dict(pixels=z["pixels"], jpg=z["jpg"].tobytes(), decoded=z["decoded"] if "decoded" in z.files else None, mode=name.split("_")[1],
                             quality=int(z["params"][0]), restart=int(z["params"][1]))
    return out


def main():
    os.makedirs(HERE, exist_ok=True)
    total = 0
    for name, (h, w, mode, q, r) in cases().items():
        a = pixels(h, w, mode)
        data = pillow_encode(a, mode, q, r)
        path = os.path.join(HERE, name + ".npz")
        arrays = dict(pixels=a, jpg=np.frombuffer(data, np.uint8), params=np.array([q, r], np.int32))
        if (h, w) in ((8, 9), (33, 50)):
            arrays["decoded"] = pillow_decode(data)
        np.savez_compressed(path, **arrays)
        total += os.path.getsize(path)
    print(f"{len(cases())} fixtures, {total} bytes")


if __name__ == "__main__":
    main()
