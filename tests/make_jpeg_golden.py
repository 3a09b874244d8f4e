"""Makes tests/golden/jpeg: the JPEG streams of the decoder's tests and the pixels Pillow (libjpeg-turbo's default decompressor) decodes
from them, ``np.asarray(Image.open(f))``; a grey stream's pixels are stored as decoded, [h, w].  Run once on the build machine:

    python -m tests.make_jpeg_golden

Every fixture is one .npz with ``jpg`` (the stream, uint8) and ``pixels`` (uint8; absent for the rejected streams).  The tests read the
committed files; tests/test_jpeg_host.py regenerates them where Pillow is importable and compares."""
import io
import os

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
SIZES = ((1, 1), (8, 9), (17, 23), (33, 50), (40, 31))            # h x w
MODES = ("grey", "444", "422", "420")
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def image(h, w, seed=0):
    """smooth sinusoids plus noise plus a saturated rectangle: clamping and every upsampling edge occur"""
    rng = np.random.default_rng(1000 * h + w + seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 110 * np.sin(x / 3.0 + c) * np.cos(y / 4.0 - 2 * c) for c in range(3)], axis=2) + rng.normal(0, 14, (h, w, 3))
    a[h // 4:h // 2 + 1, w // 4:w // 2 + 1] = (255, 0, 255)
    a[h // 2:, :max(1, w // 5)] = (0, 255, 0)
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(a, mode, quality, **kw):
    from PIL import Image
    b = io.BytesIO()
    if mode == "grey":
        Image.fromarray(a[..., 1]).save(b, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=SUBSAMPLING[mode], **kw)
    return b.getvalue()


def to_sof1_dqt16(data):
    """the same stream as SOF1 with 16-bit quantiser entries"""
    out, p = bytearray(data[:2]), 2
    while True:
        m, ln = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + ln]
        if m == 0xDB:
            body, s = bytearray(), 0
            while s < len(seg):
                assert seg[s] >> 4 == 0
                body += bytes([0x10 | (seg[s] & 15)]) + b"".join(bytes([0, v]) for v in seg[s + 1:s + 65])
                s += 65
            out += b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + body
        elif m == 0xC0:
            out += b"\xff\xc1" + data[p + 2:p + 2 + ln]
        else:
            out += data[p:p + 2 + ln]
        p += 2 + ln
        if m == 0xDA:
            return bytes(out + data[p:])


def fixtures():
    """-> {name: (stream, accepted)} in a fixed order"""
    out = {}
    for (h, w) in SIZES:
        a = image(h, w)
        for mode in MODES:
            for q in (50, 95):
                out[f"{h}x{w}_{mode}_q{q}"] = (encode(a, mode, q), True)
    a = image(33, 50)
    out["33x50_420_opt"] = (encode(a, "420", 75, optimize=True), True)
    out["33x50_420_rst2"] = (encode(a, "420", 75, restart_marker_blocks=2), True)
    out["33x50_420_rstrow"] = (encode(a, "420", 75, restart_marker_rows=1), True)
    out["33x50_420_q10"] = (encode(a, "420", 10), True)
    out["33x50_420_q100"] = (encode(a, "420", 100), True)
    out["33x50_420_sof1"] = (to_sof1_dqt16(encode(a, "420", 75)), True)
    out["75x100_420_rst1"] = (encode(image(75, 100), "420", 75, restart_marker_blocks=1), True)
    out["75x100_444_rst1"] = (encode(image(75, 100), "444", 50, restart_marker_blocks=1), True)    # 130 segments: more than 64
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(image(17, 23)).save(b, "JPEG", quality=75, progressive=True)
    out["17x23_progressive"] = (b.getvalue(), False)
    b = io.BytesIO()
    Image.fromarray(image(17, 23)).convert("CMYK").save(b, "JPEG", quality=75)
    out["17x23_cmyk"] = (b.getvalue(), False)
    return out


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def load_all():
    """the committed fixtures (no Pillow needed) -> {name: (stream bytes, RGB pixels [h, w, 3] or None for a rejected stream)}"""
    out = {}
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            z = np.load(os.path.join(HERE, f))
            px = z["pixels"] if "pixels" in z.files else None
            if px is not None and px.ndim == 2:
                px = np.stack([px, px, px], axis=2)
            out[f[:-4]] = (z["jpg"].tobytes(), px)
    return out


def main():
    os.makedirs(HERE, exist_ok=True)
    total = 0
    for name, (data, ok) in fixtures().items():
        arrays = dict(jpg=np.frombuffer(data, np.uint8))
        if ok:
            arrays["pixels"] = pillow_pixels(data)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        total += os.path.getsize(path)
    print(f"{len(fixtures())} fixtures, {total} bytes")


if __name__ == "__main__":
    main()
