"""First timing of the foreground masks of Image3D::LoadModel (csrc/grabcut.hip): 16 frames of 640 x 480 (half 320 x 240), the images
resident in HBM, through mvs_grabcut_masks_dev; wall time of the call from HIP events on its stream, the rounds every cut took
(mvs_test_grabcut_trace) and, for scale, the numpy / scipy restatement (tests/ref_grabcut.py) on the same machine's host — on a 96 x 72
frame: scipy's int32 flow cannot hold the terminal links of a 320 x 240 graph.  Per-kernel times come from running this script under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o grabcut -- python scripts/bench_grabcut.py --calls 1` (alone, no counters in the same run).
  python scripts/bench_grabcut.py [--json-out FILE]                       the measurement; prints one JSON line
  python scripts/bench_grabcut.py --report FILE [--stats CSV] --md FILE   writes the report from that line and the kernel_stats.csv
No time is a pass criterion."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.25, 0.1, 0.25, 0.1)
KERNELS = ("k_gc_half", "k_gc_start", "k_gc_thresholds", "k_gc_label0", "k_gc_ncap", "k_gc_assign", "k_gc_learn", "k_gc_fit", "k_gc_excess",
           "k_gc_update", "k_gc_full", "k_mc_seed", "k_mc_relax", "k_mc_push")


def kernel_rows(path):
    rows = []
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k + "(" in row["Name"]:
                    rows.append((k, int(row["Calls"]), int(row["TotalDurationNs"]) / 1e3))
    return sorted(rows, key=lambda r: -r[2])


def report(a):
    r = json.loads(open(a.report).read().strip().splitlines()[-1])
    out = ["# mvs_grabcut_masks: first timing", "",
           f"{r['frames']} frames of {r['w']} x {r['h']} (half {r['w'] // 2} x {r['h'] // 2}), margins {MARGINS}, gamma {r['gamma']}, {r['iters']} iterations, "
           f"images resident in HBM, `mvs_grabcut_masks_dev` on {r['device']}.", "",
           f"- call, HIP events on its stream, {len(r['call_ms'])} warm calls: {', '.join('%.2f' % v for v in r['call_ms'])} ms "
           f"(best {min(r['call_ms']):.2f} ms, {min(r['call_ms']) / r['frames']:.2f} ms per frame)",
           f"- rounds per cut (one host read per round; all frames share a cut's rounds): {r['rounds']}",
           f"- IoU of the half mask against the ellipse, per frame: min {min(r['iou']):.3f}, mean {sum(r['iou']) / len(r['iou']):.3f}",
           f"- the numpy / scipy restatement on this machine's host, one {r['ref_w']} x {r['ref_h']} frame (scipy's int32 flow cannot hold the "
           f"640 x 480 graph): {r['ref_s_per_frame'] * 1e3:.1f} ms, {r['ref_s_per_frame'] * 1e9 / (r['ref_w'] * r['ref_h'] // 4):.0f} ns per half pixel "
           f"against {min(r['call_ms']) * 1e6 / (r['frames'] * (r['w'] // 2) * (r['h'] // 2)):.1f} ns per half pixel of the call above", ""]
    if a.stats:
        rows = kernel_rows(a.stats)
        total = sum(x[2] for x in rows)
        out += ["Per kernel, summed over the three calls of a `--calls 1` run under `rocprofv3 --kernel-trace --stats` (warm-up, one timed call, the trace call):", "",
                "| kernel | launches | total us | share |", "|---|---:|---:|---:|"]
        out += [f"| {k} | {n} | {us:.1f} | {100 * us / total:.1f} % |" for k, n, us in rows]
        out += [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as fh:
        fh.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--json-out")
    ap.add_argument("--report")
    ap.add_argument("--stats")
    ap.add_argument("--md")
    a = ap.parse_args()
    if a.report:
        return report(a)
    import torch
    from multiviewstitch_amd import _lib as L, processor as P
    from tests import grabcut_scenes as SC, ref_grabcut as R
    rng = np.random.default_rng(2100)
    fr = [SC.make_frame(rng, a.w, a.h, MARGINS) for _ in range(a.frames)]
    imgs = np.ascontiguousarray(np.stack([f[0] for f in fr]))
    hl, hr, vl, vr = MARGINS
    prm = P.grabcut_params(hl=hl, hr=hr, vl=vl, vr=vr)
    st = torch.cuda.current_stream()
    dimg = torch.from_numpy(imgs).cuda()
    mask, half = P.GrabCutMasks(dimg, prm, stream=st.cuda_stream, with_half=True)      # warm-up
    half = half.cpu().numpy()
    ms = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        P.GrabCutMasks(dimg, prm, stream=st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    rounds = np.zeros(prm.iters, np.int32)
    m2 = np.zeros((a.frames, a.h, a.w), np.uint8)
    L.check(L.lib().mvs_test_grabcut_trace(a.frames, a.w, a.h, L.ptr(imgs), C.byref(prm), L.ptr(m2), None, None, None, None, None, None, L.ptr(rounds)))
    assert np.array_equal(m2, mask.cpu().numpy())
    small, _ = SC.make_frame(np.random.default_rng(2101), 96, 72, MARGINS)
    R.grabcut(small, hl, hr, vl, vr)
    t0 = time.perf_counter()
    R.grabcut(small, hl, hr, vl, vr, prm.gamma, prm.iters)
    ref_s = time.perf_counter() - t0
    line = json.dumps(dict(frames=a.frames, w=a.w, h=a.h, gamma=prm.gamma, iters=prm.iters, device=torch.cuda.get_device_name(0), call_ms=ms,
                           rounds=rounds.tolist(), iou=[SC.iou(half[f], SC.half_truth(fr[f][1])) for f in range(a.frames)],
                           ref_w=96, ref_h=72, ref_s_per_frame=ref_s))
    print(line)
    if a.json_out:
        with open(a.json_out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
