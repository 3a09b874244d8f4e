"""First timing of GeometryRec::RunPointSample on the GPU (csrc/pointsample.hip) at scan scale: 8 sequences x 16 cameras of 640 x 480, the
rasters resident in HBM, through mvs_point_sample_dev (warm: a first call sizes the capacity).  Wall time of the call from HIP events on
its stream, and in the same run mvs_check_consistency_seq_dev on the same rasters, sequence by sequence: an existing kernel with the same
gather pattern, the yardstick of the candidates launch.  Per-kernel times come from running this script under
`rocprofv3 --kernel-trace --stats -d <dir> -o pointsample -- python scripts/bench_pointsample.py` (alone, no counters in the same run);
`python scripts/bench_pointsample.py --stats <dir>/.../pointsample_kernel_stats.csv` then sums them into the candidates launch, the emit
launches, the compaction and k_check_seq.  No time is a pass criterion.  Prints one JSON line."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"candidates": ("k_ps_candidates",), "emit": ("k_ps_emit",), "compaction": ("k_ps_count", "k_ct_scan", "k_ct_strided", "k_ps_scatter"),
          "check_consistency": ("k_check_seq",)}


def summarise(path):
    out = {g: dict(calls=0, total_us=0.0) for g in GROUPS}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for g, names in GROUPS.items():
                if any(n + "(" in row["Name"] for n in names):
                    out[g]["calls"] += int(row["Calls"])
                    out[g]["total_us"] += int(row["TotalDurationNs"]) / 1e3
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 run of this script: print the per-group sums and exit")
    a = ap.parse_args()
    if a.stats:
        return summarise(a.stats)
    import torch
    from multiviewstitch_amd import processor as P, scene as S
    cameras, depths = [], []
    for k in range(a.seqs):                                                           # two surfaces, taken in turn (the ray caster is slow)
        if k < 2:
            cams, d = S.make_sequence(n_frames=a.frames, w=a.w, h=a.h, dyaw_deg=3.0, seed=77 + k, device="cuda")
            depths.append(torch.as_tensor(d, dtype=torch.float32, device="cuda").contiguous())
        else:
            cams = cameras[k - 2]
            depths.append(depths[k - 2].clone())
        cameras.append(cams)
    prm = P.point_sample_params(dsp_min=S.MIN_DSP, dsp_max=S.MAX_DSP, max_dsp_err=0.002)
    st = torch.cuda.current_stream()
    flat = torch.cat([d.reshape(-1) for d in depths])                                 # all rasters back to back: read in place
    res = P.RunPointSample(cameras, flat, prm, stream=st.cuda_stream)                 # warm-up; sizes the capacity
    points = sum(len(r[0]) for r in res)

    def timed(fn):
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    call_ms = timed(lambda: P.RunPointSample(cameras, flat, prm, stream=st.cuda_stream, capacity=points))
    out = [torch.empty_like(d) for d in depths]

    def check():
        for c, d, o in zip(cameras, depths, out):
            P.CheckConsistency(c, int(d.data_ptr()), S.MIN_DSP, S.MAX_DSP, 2, out_dev=int(o.data_ptr()), stream=st.cuda_stream)

    check()
    check_ms = timed(check)
    valid = sum(int(((d >= S.MIN_DSP) & (d <= S.MAX_DSP)).sum()) for d in depths)
    print(json.dumps(dict(seqs=a.seqs, frames=a.frames, w=a.w, h=a.h, pt_samp_rds=prm.pt_samp_rds, nbr_frm_num=prm.nbr_frm_num, valid_pixels=valid,
                          points=points, call_ms=call_ms, call_ms_best=min(call_ms), check_consistency_ms=check_ms,
                          check_consistency_ms_best=min(check_ms), raster_bytes=4 * a.seqs * a.frames * a.w * a.h)))


if __name__ == "__main__":
    main()
