"""Times the stitch tail of Processor::AlignmentSeq at scan scale (8 sequences x 16 cameras, ~2 M points):

  * the visibility cull (mvs_visibility_cull_dev, MVS_CULL_SEQUENCES) with the points resident in HBM;
  * mvs_processor_stitch_points end to end (8 .npts files -> PSR%d.obj + PSR.npts).

Run it under `rocprofv3 --kernel-trace --stats -d <dir> -o stitch -- python scripts/bench_stitch.py` for the kernel time of
k_vis_cull; the script itself prints one JSON line with host-clock times (every call ends in a device synchronise), the
projections per second, the bytes the cull moves and the two floors (fp64 VALU and HBM).

Floors.  A projection (camera_dev.h img_from_world + CheckRange) is 52 fp64 VALU instructions in the gfx950 ISA of k_vis_cull:
13 v_mul_f64, 13 v_add_f64, 10 v_fma/v_fmac_f64 + 4 v_div_scale + 2 v_rcp + 2 v_div_fmas + 2 v_div_fixup (the two IEEE divides),
2 v_cvt_i32_f64, 4 v_cmp_*_f64.  The FP64 vector rate is AMD's published MI355X figure, 78.6 TFLOP/s with an FMA counted as
2 FLOP, i.e. 39.3e12 fp64 lane-instructions per second (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).  The cull reads 24 B per point
and writes its mask byte (~25 B / point); HBM peak 8.0 TB/s (6.29 TB/s measured copy, MI355X_MICROARCH).  Wave-level early exit
means a culled wave stops projecting; the fp64 floor below counts every projection (no exit), so it is an upper bound of the
work and the measured rate is given against the same count."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_INSTR_PER_PROJ = 52
FP64_LANE_INSTR_PER_S = 78.6e12 / 2
HBM_BPS = 8.0e12


def inputs(n_seq, cams, per, seed=9):
    from multiviewstitch_amd import scene as S
    from multiviewstitch_amd import srt
    scales, Rs, ts, cameras = S.make_stitch_sequences([cams] * n_seq, [(1280, 960)] * n_seq, [2.2] * n_seq, seed=21)
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for k in range(n_seq):
        d = rng.normal(size=(per, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        w = np.ascontiguousarray(d * rng.uniform(0.85, 1.15, (per, 1)))
        lp, ln = srt.apply(w, d, scales[k], Rs[k], ts[k], inverse=True)
        pts.append(lp)
        nrm.append(ln)
    return scales, Rs, ts, cameras, pts, nrm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e-reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from multiviewstitch_amd import _lib, processor, srt
    from multiviewstitch_amd import io as mio
    if _lib.device_count() == 0:
        raise SystemExit("bench_stitch needs a GPU: libmvs_hip has no CPU fallback")
    per = args.points // args.seqs
    scales, Rs, ts, cameras, pts, nrm = inputs(args.seqs, args.cams, per)
    allp = np.concatenate(pts)
    P = len(allp)
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    dp = torch.from_numpy(allp).to("cuda")
    dk = torch.empty(P, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):                                                # warm: code object, scratch pool
        nk = srt.visibility_cull_dev(dp.data_ptr(), off, scales, Rs, ts, cameras, dk.data_ptr())
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        nk = srt.visibility_cull_dev(dp.data_ptr(), off, scales, Rs, ts, cameras, dk.data_ptr())
        times.append(time.perf_counter() - t0)
    cull_s = float(np.median(times))
    n_proj = P * args.seqs * args.cams                                # every point against every camera (no early exit)
    fp64_floor = n_proj * FP64_INSTR_PER_PROJ / FP64_LANE_INSTR_PER_S
    bytes_moved = P * 25
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k in range(args.seqs):
            paths.append(os.path.join(d, f"seq{k}.npts"))
            mio.write_npts(paths[-1], pts[k], nrm[k])
        out = os.path.join(d, "out")
        os.mkdir(out)
        processor.StitchPointSets(paths, scales, Rs, ts, cameras, out)   # warm
        e2e = []
        for _ in range(args.e2e_reps):
            t0 = time.perf_counter()
            processor.StitchPointSets(paths, scales, Rs, ts, cameras, out)
            e2e.append(time.perf_counter() - t0)
    res = {
        "what": "stitch tail at scan scale", "points": P, "sequences": args.seqs, "cameras_per_sequence": args.cams,
        "kept_fraction": float(nk.sum() / P),
        "cull_call_ms_median": cull_s * 1e3, "cull_call_ms_min": min(times) * 1e3,
        "projections_nominal": n_proj, "projections_per_s_nominal": n_proj / cull_s,
        "bytes": bytes_moved, "hbm_floor_us": bytes_moved / HBM_BPS * 1e6,
        "fp64_floor_us": fp64_floor * 1e6, "bound": "fp64 VALU" if fp64_floor > bytes_moved / HBM_BPS else "HBM",
        "stitch_points_e2e_ms_median": float(np.median(e2e)) * 1e3,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
