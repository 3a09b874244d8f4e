"""First timing of FeatureProc::DetectFeature on the GPU (csrc/sift.hip) at the shape of `main -a 1`: 16 frames x 3 views of 640 x 480,
first_octave = -1, the rasters resident in HBM, through mvs_sift_detect_dev.  Wall time of the call (HIP events on its stream, after a
warm-up call) and the key count; per-kernel times come from running this script under `rocprofv3 --kernel-trace --stats -- python
scripts/bench_sift.py` (alone, no counters in the same run).  The blur's achieved bandwidth is its algorithmic bytes (every Gaussian
level the blur makes, read once and written once, 8 bytes per pixel) over the summed time of k_sift_blur from the kernel stats; it is put beside the
copy ceiling `bench.py --full` reports.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def content(n, w, h, seed=1):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        a = np.full((h, w), 0.45, np.float32)
        for _ in range(400):
            cx, cy, s = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1.2, 6.0)
            x0, x1, y0, y1 = int(max(0, cx - 4 * s)), int(min(w, cx + 4 * s + 1)), int(max(0, cy - 4 * s)), int(min(h, cy + 4 * s + 1))
            a[y0:y1, x0:x1] += rng.uniform(0.1, 0.4) * rng.choice([-1, 1]) * np.exp(-((xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2) / (2 * s * s))
        a += rng.normal(0, 0.004, (h, w)).astype(np.float32)
        out[i] = np.clip(a * 255, 0, 255).astype(np.uint8)[..., None]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    import torch
    from multiviewstitch_amd import processor as P
    n = a.frames * a.views
    imgs = torch.from_numpy(content(n, a.w, a.h)).cuda()
    prm = P.sift_params(first_octave=-1)
    st = torch.cuda.current_stream()
    off, keys, _ = P.DetectFeature(imgs, prm, stream=st.cuda_stream)                  # warm-up; sizes the capacity
    cap = int(off[-1])
    ms = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        off, keys, _ = P.DetectFeature(imgs, prm, stream=st.cuda_stream, capacity=cap)
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    px, W, H = 0, 2 * a.w, 2 * a.h
    from tests import ref_sift as R
    for o in range(R.octaves(W, H)):                                                  # sizes halve with integer division, as rule 4
        # S + 3 levels per octave; level 0 of every octave after the first is written by k_sift_down, not by the blur
        px += (prm.dog_levels + 3 - (1 if o else 0)) * (W >> o) * (H >> o)
    print(json.dumps(dict(lists=n, w=a.w, h=a.h, first_octave=-1, keys=cap, keys_per_list=cap / n, call_ms=ms, call_ms_best=min(ms),
                          blur_algorithmic_bytes=8 * px * n)))


if __name__ == "__main__":
    main()
