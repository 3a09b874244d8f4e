"""Times the match-filter cascade of one sequence pair at the shape of `main -a 1` (16 x 16 frame pairs of 640 x 480 images, 5
generated views per frame, about 3 000 raw matches per pair):

  (a) the loop that existed before: mvs_match_filter once per frame pair (the stage-1 rule on the host, then the cascade kernel of
      (b) as its 1 x 1 case; the keys and both base images uploaded and the stream synchronised at every call);
  (b) mvs_match_filter_pairs: all 256 pairs in one call (matchpairs.hip; every stack uploaded once);
  (c) mvs_match_filter_pairs_dev: the same with the stacks already in HBM.

Every repetition is timed on the host clock (each call returns with its work complete) and runs under its own time limit; the
script prints one JSON line with the median, the minimum and the spread (max - min) of the repetitions, and whether (a) and (b)
agree bit for bit.  Run it under `rocprofv3 --kernel-trace --stats -d <dir> -o matchpairs -- python scripts/bench_matchpairs.py`
for the kernel times."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(n1, n2, w, h, views, n_raw, seed=0):
    """Per frame: a smooth image with noise, texIndex tables that are one-pixel shifts of the identity with 5 % holes, a valid mask
    with 5 % holes.  Per pair: true correspondences (image 2 = image 1 moved 4 px) with 20 % gross errors, 10 % duplicates and a few
    out-of-range pixels, each seen in a random generated view."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 96 + 60 * np.sin(xx / 17.0) * np.cos(yy / 13.0) + 30 * np.sin((xx + 2 * yy) / 29.0)
    idx = (yy * w + xx).astype(np.int32)
    shifts = [(0, 0), (1, 1), (-1, 0), (2, 1), (-2, 0)]
    tex0 = np.stack([idx if s == 0 else np.roll(idx, s, axis=a) for s, a in (shifts * views)[:views]]).reshape(views, -1)

    def frames(n, shift):
        imgs = np.empty((n, h, w, 3), np.uint8)
        tex = np.empty((n, views, w * h), np.int32)
        valid = np.empty((n, w * h), np.uint8)
        for k in range(n):
            b = np.roll(base, shift, axis=1)
            imgs[k] = np.clip(np.stack([b, b * 0.8 + 20, 255 - b], -1) + rng.normal(scale=2, size=(h, w, 3)), 0, 255).astype(np.uint8)
            tex[k] = tex0
            tex[k][:, rng.random(w * h) < 0.05] = -1
            valid[k] = rng.random(w * h) > 0.05
        return tex, valid, imgs

    tex1, valid1, imgs1 = frames(n1, 0)
    tex2, valid2, imgs2 = frames(n2, 4)
    raw = []
    for i in range(n1):
        row = []
        for j in range(n2):
            n = int(n_raw * 0.9)
            u1, v1 = rng.integers(-2, w + 2, n), rng.integers(-2, h + 2, n)
            u2 = u1 + 4 + np.where(rng.random(n) < 0.2, rng.integers(-40, 41, n), 0)
            v2 = v1 + np.where(rng.random(n) < 0.2, rng.integers(-30, 31, n), 0)
            r = np.stack([rng.integers(0, views, n), u1, v1, rng.integers(0, views, n), u2, v2], 1).astype(np.int32)
            row.append(np.concatenate([r, r[:n_raw - n]]))
        raw.append(row)
    return raw, tex1, valid1, tex2, valid2, imgs1, imgs2


class Limit:
    """a time limit of its own for every repetition (SIGALRM: the call is host code that waits for the device)"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)

    def _fire(self, *_):
        raise TimeoutError(f"a repetition ran longer than {self.seconds} s")


def timed(fn, reps, warm, limit):
    for _ in range(warm):                                         # code objects, scratch pool
        with Limit(limit):
            fn()
    t = []
    for _ in range(reps):
        with Limit(limit):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    return t


def stats(t):
    return {"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3, "spread_ms": (max(t) - min(t)) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=16)
    ap.add_argument("--n2", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--raw", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=60, help="seconds allowed to one repetition")
    ap.add_argument("--ssd-win", type=int, default=3)
    ap.add_argument("--ssd-err", type=float, default=6.0)
    ap.add_argument("--interval", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 timed repetitions")
    import torch
    from multiviewstitch_amd import _lib, processor
    if _lib.device_count() == 0:
        raise SystemExit("bench_matchpairs needs a GPU: libmvs_hip has no CPU fallback")
    raw, tex1, valid1, tex2, valid2, imgs1, imgs2 = inputs(args.n1, args.n2, args.w, args.h, args.views, args.raw)
    flt = (args.ssd_win, args.ssd_err, args.interval)
    res_a, res_b = {}, {}

    def loop():                                                   # (a)
        for i in range(args.n1):
            for j in range(args.n2):
                res_a[i, j] = processor.MatchFilter(raw[i][j], tex1[i], valid1[i], tex2[j], valid2[j], imgs1[i], imgs2[j], *flt)

    def batched():                                                # (b)
        res_b["out"] = processor.MatchFilterPairs(raw, tex1, valid1, tex2, valid2, imgs1, imgs2, *flt)

    dev = [torch.from_numpy(a).to("cuda") for a in (tex1, valid1, tex2, valid2, imgs1, imgs2)]
    torch.cuda.synchronize()

    def batched_dev():                                            # (c)
        processor.MatchFilterPairs(raw, *dev, *flt)

    ta = timed(loop, args.reps, args.warmup, args.limit)
    tb = timed(batched, args.reps, args.warmup, args.limit)
    tc = timed(batched_dev, args.reps, args.warmup, args.limit)
    got, cnt = res_b["out"]
    same = all(np.array_equal(got[i][j], res_a[i, j][0]) and np.array_equal(cnt[i, j], res_a[i, j][1])
               for i in range(args.n1) for j in range(args.n2))
    a, b, c = stats(ta), stats(tb), stats(tc)
    print(json.dumps({
        "what": "match-filter cascade of one sequence pair", "pairs": args.n1 * args.n2, "w": args.w, "h": args.h, "views": args.views,
        "raw_per_pair": args.raw, "ssd_win": args.ssd_win, "ssd_err": args.ssd_err, "sample_interval": args.interval,
        "reps": args.reps, "warmup": args.warmup, "stage_counts_mean": [float(x) for x in cnt.reshape(-1, 3).mean(0)],
        "a_equals_b": bool(same), "a_loop_of_mvs_match_filter": a, "b_mvs_match_filter_pairs": b, "c_mvs_match_filter_pairs_dev": c,
        "speedup_b_over_a": a["median_ms"] / b["median_ms"],
        "b_faster_beyond_spread": bool(b["max_ms"] < a["min_ms"]),
    }))


if __name__ == "__main__":
    main()
