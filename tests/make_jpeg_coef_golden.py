"""Makes tests/golden/jpeg_coef: the streams ``ref_jpeg_enc.encode_coef`` writes from the coefficient cases of tests/jpeg_coef_cases.py that
Pillow decodes as the rules do (``GOLDEN`` there: ff, sym, zrl and rand in every mode, long once; all at quality 100, where every
quantiser is 1 and libjpeg-turbo's 16-bit intermediates hold what rule J4 computes), and the pixels Pillow (libjpeg-turbo's default
decompressor) decodes from them, ``np.asarray(Image.open(f))``; a grey stream's pixels are stored as decoded, [h, w].  Run once on the
build machine:

    python -m tests.make_jpeg_coef_golden

Every fixture is one .npz with ``jpg`` (the stream, uint8) and ``pixels`` (uint8).  The tests read the committed files;
tests/test_jpeg_coef_host.py regenerates them where Pillow is importable and compares."""
import os

import numpy as np

from tests import jpeg_coef_cases as K
from tests.make_jpeg_golden import pillow_pixels

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_coef")


def fixtures():
    """-> {name: (stream, the pixels Pillow decodes from it)}"""
    return {name: (K.encoded(name)[0], pillow_pixels(K.encoded(name)[0])) for name in K.GOLDEN}


def load_all():
    """the committed fixtures (no Pillow needed) -> {name: (stream bytes, RGB pixels [h, w, 3])}"""
    out = {}
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            z = np.load(os.path.join(HERE, f))
            px = z["pixels"]
            out[f[:-4]] = (z["jpg"].tobytes(), np.stack([px, px, px], axis=2) if px.ndim == 2 else px)
    return out


def main():
    os.makedirs(HERE, exist_ok=True)
    total = 0
    for name, (data, px) in fixtures().items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, jpg=np.frombuffer(data, np.uint8), pixels=px)
        total += os.path.getsize(path)
    print(f"{len(K.GOLDEN)} fixtures, {total} bytes")


if __name__ == "__main__":
    main()
