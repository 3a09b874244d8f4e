"""First timing of the head of Processor::CalcSimilarityTransformationSeq on the GPU, at the shape of `main -a 1`: 8 sequences of 16
frames, 640 x 480, view_count 3, 4 000 key points per generated view.

  (a) mvs_gen_new_views_dev, one call per sequence (images and outputs in HBM);
  (b) mvs_keypoint_cull_dev, one call per sequence (48 lists of 4 000 keys with their descriptors, everything in HBM);
  (c) the numpy restatement of GenNewViews (tests/ref_views.py) on ONE frame of the same size — the only CPU figure there is.

(a) and (b) are timed with HIP events on the stream the call works on, after a warm-up, each call under its own time limit; a call
returns with its work complete, so the events bracket host work too.  The bytes (a) writes (views and tex) over its time are put
beside the device-to-device copy ceiling, measured here the way `bench.py --full` measures it (1 GiB copies, read + write bytes);
that rate is of the whole call, bounding-box pass included, so it is a lower bound for the paint.  Prints one JSON line."""
import argparse
import json
import math
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Limit:
    """a time limit of its own for every call (SIGALRM: the call is host code that waits for the device)"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)

    def _fire(self, *_):
        raise TimeoutError(f"a call ran longer than {self.seconds} s")


def stats(t):
    return {"median_us": float(np.median(t)), "min_us": float(min(t)), "max_us": float(max(t)), "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--keys", type=int, default=4000)
    ap.add_argument("--rot", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=60, help="seconds allowed to one call")
    args = ap.parse_args()
    import torch
    from multiviewstitch_amd import _lib, processor, scene as S
    from tests import ref_views as RV
    if _lib.device_count() == 0:
        raise SystemExit("bench_views needs a GPU: libmvs_hip has no CPU fallback")
    w, h, n, vc = args.w, args.h, args.frames, args.views
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w]
    seqs = []
    for k in range(args.sequences):
        cams = []
        for f in range(n):                                        # a ring of cameras looking at the origin, 3 degrees apart
            yaw = math.radians(3.0) * (k * n + f)
            Rc, tc = S._look_at(5.0 * np.array([math.cos(yaw), math.sin(yaw), 0.17]))
            cams.append(S.Camera(1.2 * w, 1.2 * w, w / 2 - 0.5, h / 2 - 0.5, Rc, tc, w, h))
        base = 128 + 60 * np.sin(xx / 9.0 + k) * np.cos(yy / 7.0)
        imgs = np.clip(np.stack([base, 0.8 * base + 20, 255 - base], -1)[None] + rng.normal(scale=2, size=(n, h, w, 3)), 0, 255).astype(np.uint8)
        depths = np.full((n, h * w), 0.2, np.float32)             # a fronto-parallel sheet 5 units away: every pixel valid
        keys = np.stack([rng.uniform(0, w, n * vc * args.keys), rng.uniform(0, h, n * vc * args.keys), rng.uniform(1, 8, n * vc * args.keys),
                         rng.uniform(-3, 3, n * vc * args.keys)], 1).astype(np.float32)
        descs = rng.random((n * vc * args.keys, 128), dtype=np.float32)
        seqs.append(dict(cams=cams, imgs=torch.from_numpy(imgs).to("cuda"), depths=torch.from_numpy(depths).to("cuda"),
                         keys=torch.from_numpy(keys).to("cuda"), descs=torch.from_numpy(descs).to("cuda"), frame0=imgs[0]))
    off = np.arange(n * vc + 1, dtype=np.int64) * args.keys
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()

    def event_timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with Limit(args.limit):
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
        return out, 1e3 * e0.elapsed_time(e1)

    tv, tc, kept = [], [], 0
    for rep in range(args.warmup + args.reps):
        for q in seqs:
            (views, tex), us = event_timed(lambda: processor.GenNewViews(q["cams"], q["imgs"], vc, 0, args.rot, stream=stream.cuda_stream))
            q["tex"] = tex
            r, us2 = event_timed(lambda: processor.KeypointCull(q["cams"], vc, off, q["keys"], q["descs"], q["tex"], q["depths"], S.MIN_DSP, S.MAX_DSP,
                                                                stream=stream.cuda_stream))
            if rep >= args.warmup:
                tv.append(us); tc.append(us2); kept = int(r["out_offsets"][-1])
    a = torch.empty(1 << 27, dtype=torch.float64, device="cuda").normal_()        # 1 GiB each way, as bench.py --full
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_gbps = 10 * 2 * a.numel() * 8 / (1e-3 * e0.elapsed_time(e1)) / 1e9
    del a, b
    t0 = time.perf_counter()
    RV.gen_new_views(seqs[0]["cams"][:1], seqs[0]["frame0"][None], vc, 0, args.rot)
    cpu_s = time.perf_counter() - t0
    written = n * vc * w * h * (3 + 4)
    sv, sc = stats(tv), stats(tc)
    print(json.dumps({
        "what": "GenNewViews and the key-point cull of one sequence, device forms", "sequences": args.sequences, "frames": n, "w": w, "h": h,
        "view_count": vc, "keys_per_view": args.keys, "reps": args.reps, "warmup": args.warmup,
        "a_mvs_gen_new_views_dev": sv, "b_mvs_keypoint_cull_dev": sc, "keys_per_call": int(off[-1]), "kept_per_call": kept,
        "a_bytes_written_per_call": written, "a_written_GBps_of_whole_call": written / (sv["median_us"] * 1e-6) / 1e9,
        "copy_ceiling_GBps": copy_gbps, "c_numpy_restatement_one_frame_s": cpu_s,
        "c_numpy_restatement_per_sequence_s_extrapolated": cpu_s * n,
    }))


if __name__ == "__main__":
    main()
