"""Times Processor::Render's depth renders at the shape of `main -a 0` (8 sequences x 16 cameras at 640x480, the config-3
template of 54 762 vertices in HBM):

  (a) the per-view path that existed before: per sequence mvs_srt_apply_dev (inverse map), then mvs_render_depth_dev per camera;
  (b) mvs_render_depth_views_dev: all 128 views in one call (binned tile rasterizer, render_views.hip);
  (c) mvs_processor_render end to end (deform.obj + SRT.txt -> render%d.obj + 128 _depth%d.raw files).

Run it under `rocprofv3 --kernel-trace --stats -d <dir> -o render -- python scripts/bench_render.py` for the kernel times; the
script prints one JSON line with host-clock times (every call ends in a device synchronise), whether (a) and (b) agree bit for
bit, and the fp64-VALU floor of the (triangle, pixel) tests.

Floor.  A (triangle, pixel) test of rd_pixel (render_dev.h) is FP64_INSTR_PER_TEST fp64 VALU instructions on the path where the
centre is outside (the common case): two int -> double conversions and two adds for the centre, three edge functions of two
subtracts, two multiplies and one subtract each (the edge vectors are per triangle), and the compares of the top-left rule.
The count of tests is every pixel of every accepted triangle's clamped range, evaluated here in float64 (a floor, not a bit-exact
count).  The FP64 vector rate is AMD's published MI355X figure, 78.6 TFLOP/s with an FMA counted as 2 FLOP, i.e. 39.3e12 fp64
lane-instructions per second."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_INSTR_PER_TEST = 25
FP64_LANE_INSTR_PER_S = 78.6e12 / 2


def inputs(n_seq, cams, w, h, f):
    from multiviewstitch_amd import scene as S
    sc = S.make_scene(3, views=[])                            # the template only (no depth maps)
    scales, Rs, ts, cameras = S.make_stitch_sequences([cams] * n_seq, [(w, h)] * n_seq, [f] * n_seq, seed=21)
    return sc.verts.copy(), sc.faces.astype(np.int32), scales, Rs, ts, cameras


def count_tests(pts, faces, scales, Rs, ts, cameras, znear=0.01):
    """(triangle, pixel) tests of every view: the clamped pixel ranges of the triangles in front of the eye plane (float64)."""
    n = 0
    for k, seq in enumerate(cameras):
        q = (Rs[k].T @ (pts - ts[k]).T).T / scales[k]
        for c in seq:
            pc = q @ np.asarray(c.R).T + np.asarray(c.t)
            z = pc[:, 2]
            with np.errstate(all="ignore"):
                x = c.fx * pc[:, 0] / z + c.cx + 0.5          # window x (GL's y is flipped; the range sizes are the same)
                y = c.fy * pc[:, 1] / z + c.cy + 0.5
            A, B, C = faces[:, 0], faces[:, 1], faces[:, 2]
            ok = (z[A] > znear) & (z[B] > znear) & (z[C] > znear)
            xs, ys = np.stack([x[A], x[B], x[C]])[:, ok], np.stack([y[A], y[B], y[C]])[:, ok]
            i0 = np.clip(np.floor(xs.min(0) - 0.5), 0, c.w - 1)
            i1 = np.clip(np.ceil(xs.max(0) - 0.5), 0, c.w - 1)
            j0 = np.clip(np.floor(ys.min(0) - 0.5), 0, c.h - 1)
            j1 = np.clip(np.ceil(ys.max(0) - 0.5), 0, c.h - 1)
            inside = (xs.max(0) >= 0) & (xs.min(0) <= c.w) & (ys.max(0) >= 0) & (ys.min(0) <= c.h)
            n += int(((i1 - i0 + 1) * (j1 - j0 + 1))[inside].sum())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--f", type=float, default=1.4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e-reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from multiviewstitch_amd import _lib, processor, srt
    from multiviewstitch_amd import io as mio
    if _lib.device_count() == 0:
        raise SystemExit("bench_render needs a GPU: libmvs_hip has no CPU fallback")
    pts, faces, scales, Rs, ts, cameras = inputs(args.seqs, args.cams, args.w, args.h, args.f)
    V, F, N = len(pts), len(faces), args.seqs * args.cams
    dp, df = torch.from_numpy(pts).to("cuda"), torch.from_numpy(faces).to("cuda")
    mapped = [torch.empty_like(dp) for _ in range(args.seqs)]
    out_a = torch.empty((N, args.h, args.w), dtype=torch.float32, device="cuda")
    out_b = torch.empty_like(out_a)
    torch.cuda.synchronize()

    def loop():                                                       # (a)
        v = 0
        for k in range(args.seqs):
            srt.apply_dev(dp.data_ptr(), None, V, scales[k], Rs[k], ts[k], mapped[k].data_ptr(), None, inverse=True)
            for c in cameras[k]:
                processor.RenderDepth((mapped[k].data_ptr(), V), (df.data_ptr(), F), c, out_dev=out_a[v].data_ptr())
                v += 1

    def batched():                                                    # (b)
        processor.RenderViews((dp.data_ptr(), V), (df.data_ptr(), F), cameras, scales, Rs, ts, out_dev=out_b.data_ptr())

    def timed(fn, reps):
        for _ in range(2):                                            # warm: code objects, scratch pool
            fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return t

    ta = timed(loop, args.reps)
    tb = timed(batched, args.reps)
    same = bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)))
    covered = float((out_b > 0).float().mean())
    with tempfile.TemporaryDirectory() as d:
        res = os.path.join(d, "Result")
        os.mkdir(res)
        mio.WriteObj(os.path.join(res, "deform.obj"), pts, None, faces)
        mio.write_srt_txt(os.path.join(res, "SRT.txt"), scales, Rs, ts)
        dirs = [os.path.join(d, f"seq{k}") for k in range(args.seqs)]
        tc = timed(lambda: processor.Render(os.path.join(res, "deform.obj"), os.path.join(res, "SRT.txt"), cameras, res, dirs),
                   args.e2e_reps)
    tests = count_tests(pts, faces, scales, Rs, ts, cameras)
    floor = tests * FP64_INSTR_PER_TEST / FP64_LANE_INSTR_PER_S
    res = {
        "what": "Processor::Render depth renders", "views": N, "sequences": args.seqs, "cameras_per_sequence": args.cams,
        "w": args.w, "h": args.h, "vertices": V, "faces": F, "covered_fraction": covered, "a_equals_b": same,
        "a_per_view_loop_ms_median": float(np.median(ta)) * 1e3, "a_per_view_loop_ms_min": min(ta) * 1e3,
        "b_render_views_ms_median": float(np.median(tb)) * 1e3, "b_render_views_ms_min": min(tb) * 1e3,
        "c_processor_render_e2e_ms_median": float(np.median(tc)) * 1e3,
        "speedup_b_over_a": float(np.median(ta) / np.median(tb)),
        "tests_triangle_pixel": tests, "fp64_floor_us": floor * 1e6,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
