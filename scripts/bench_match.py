"""First timing of FeatureProc::MatchFeature on the GPU (csrc/siftmatch.hip) at the shape of `main -a 1`: 2 adjacent sequences of 16
frames, view_count 5, about 1 000 key points per generated view: 80 x 80 = 6 400 list pairs of 1 000 x 1 000 x 128.

  (a) mvs_sift_match_lists_dev, one call for all list pairs (keys and descriptors in HBM, the rows come back to the host);
  (b) a loop of mvs_sift_match over the same 6 400 list pairs, the way the reference calls SiftMatchGPU (host arrays);
  (c) a torch baseline per list pair on the same quantised bytes: an fp16 matmul (exact here: integers up to 255, sums below 2^24)
      and its row and column maxima — no second-best, no thresholds, no rows: less than (a) computes.

(a) and (c) are timed with HIP events on the stream they work on, after a warm-up; (b) is host code that uploads per call and is
timed with the wall clock; every timed call runs under its own time limit.  The integer-op rate of (a) counts 2 * 128 operations per
score and BOTH directions (the kernel computes each score twice), over the whole call, uploads of tables and the download
of the rows included; the i8 MFMA peak it is put beside is twice the dense bf16 figure.  Prints one JSON line."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

I8_PEAK_OPS = 2 * 2.5e15                                            # i8 MFMA: twice the bf16 rate per clock; bf16 ~2.5 PF dense


class Limit:
    """a time limit of its own for every timed stretch (SIGALRM: the calls are host code that waits for the device)"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)

    def _fire(self, *_):
        raise TimeoutError(f"a timed stretch ran longer than {self.seconds} s")


def stats(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-reps", type=int, default=1, help="repetitions of the 6 400-call loops (b) and (c)")
    ap.add_argument("--limit", type=int, default=120, help="seconds allowed to one timed stretch")
    args = ap.parse_args()
    import torch
    from multiviewstitch_amd import _lib, processor
    from tests import ref_match as RM
    from tests.test_match_feature_host import noisy, random_keys, sift_like
    if _lib.device_count() == 0:
        raise SystemExit("bench_match needs a GPU: libmvs_hip has no CPU fallback")
    n, vc, L = args.frames, args.views, args.frames * args.views
    rng = np.random.default_rng(0)
    lens1 = rng.integers(int(0.9 * args.keys), int(1.1 * args.keys) + 1, L)
    lens2 = rng.integers(int(0.9 * args.keys), int(1.1 * args.keys) + 1, L)
    pool = sift_like(rng, int(1.1 * args.keys) + 1)                  # every list sees the same surface: copies of one pool
    descs1 = [noisy(rng, pool[rng.permutation(len(pool))[:m]], 0.03) for m in lens1]
    descs2 = [noisy(rng, pool[rng.permutation(len(pool))[:m]], 0.03) for m in lens2]
    keys1, keys2 = [random_keys(rng, m) for m in lens1], [random_keys(rng, m) for m in lens2]
    off1, off2 = np.concatenate([[0], np.cumsum(lens1)]).astype(np.int64), np.concatenate([[0], np.cumsum(lens2)]).astype(np.int64)
    dev = [torch.from_numpy(np.concatenate(a)).to("cuda") for a in (keys1, descs1, keys2, descs2)]
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    scores = float(np.outer(lens1, lens2).sum())

    def batched():
        return processor.MatchFeature(dev[0], dev[1], dev[2], dev[3], vc, stream=stream.cuda_stream, key_offsets1=off1, key_offsets2=off2)

    ta, raw = [], None
    for rep in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with Limit(args.limit):
            e0.record(stream)
            raw = batched()
            e1.record(stream)
            e1.synchronize()
        if rep >= args.warmup:
            ta.append(e0.elapsed_time(e1))
    matches = int(sum(len(b) for row in raw for b in row))

    tb, loop_matches = [], 0
    processor.MatchFeatureSingleView(descs1[0], descs2[0])
    for _ in range(args.loop_reps):
        with Limit(args.limit):
            t0 = time.perf_counter()
            loop_matches = sum(len(processor.MatchFeatureSingleView(a, b)) for a in descs1 for b in descs2)
            tb.append(1e3 * (time.perf_counter() - t0))

    q1 = [torch.from_numpy(RM.quantise(d).astype(np.float16)).to("cuda") for d in descs1]
    q2 = [torch.from_numpy(RM.quantise(d).astype(np.float16)).to("cuda") for d in descs2]
    torch.cuda.synchronize()
    tc, check = [], 0.0
    for rep in range(1 + args.loop_reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with Limit(args.limit):
            e0.record(stream)
            for a in q1:
                for b in q2:
                    s = a @ b.T
                    r, c = s.max(dim=1), s.max(dim=0)
            e1.record(stream)
            e1.synchronize()
        check = float(r.values.float().sum() + c.values.float().sum())
        if rep >= 1:
            tc.append(e0.elapsed_time(e1))

    sa, sb, sc = stats(ta), stats(tb), stats(tc)
    ops = 2 * 2 * 128 * scores
    print(json.dumps({
        "what": "descriptor matching of one sequence pair", "frames": n, "view_count": vc, "keys_per_list": args.keys, "list_pairs": L * L,
        "scores_per_direction": scores, "matches": matches, "loop_matches": int(loop_matches), "a_equals_b_in_count": matches == loop_matches,
        "a_mvs_sift_match_lists_dev": sa, "b_loop_of_mvs_sift_match": sb, "c_torch_fp16_matmul_and_max_per_pair": sc,
        "a_integer_ops": ops, "a_Tops_of_whole_call": ops / (sa["median_ms"] * 1e-3) / 1e12,
        "a_fraction_of_i8_mfma_peak": ops / (sa["median_ms"] * 1e-3) / I8_PEAK_OPS, "i8_peak_ops_assumed": I8_PEAK_OPS,
        "b_over_a": sb["median_ms"] / sa["median_ms"], "c_over_a": sc["median_ms"] / sa["median_ms"], "c_checksum": check,
    }))


if __name__ == "__main__":
    main()
