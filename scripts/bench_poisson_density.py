"""Timing of the sampling-density rules of the Poisson stage (csrc/poisson.hip and, the trim, csrc/mesh_trim.hip; rules 14-18 of include/mvs.h) with the set-up of
scripts/bench_poisson.py: 2 M oriented points on a rotated ellipsoid (semi-axes 1, 0.7, 0.5), resident in HBM, depth 8 and depth 9
(depth_min = depth_max).  Per depth, from HIP events on the call's stream, three calls after a warm-up each: the plain call
(mvs_poisson_reconstruct_dev) and, in the same run, the call with the weighting and the vertex density
(mvs_poisson_reconstruct_density_dev); their spread (max - min over the calls) is the run-to-run spread the comparison has to respect.
Then the trim (mvs_mesh_trim_by_value_dev) of the depth-9 mesh at 0.25 x the mean point density.  Per-kernel times come from running
this script under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o density -- python scripts/bench_poisson_density.py
--depths 9 --calls 1` (alone, no counters in the same run); `python scripts/bench_poisson_density.py --stats <dir>/.../density_kernel_stats.csv`
then groups the new kernels.  No time is a pass criterion.  Prints one JSON line."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"density_splat": ("k_pn_density_splat",), "point_density": ("k_pn_point_density",), "gain": ("k_pn_gain",),
          "splat_weighted": ("void (anonymous namespace)::k_pn_splat<true>", "k_pn_splat<true>"),
          "splat_plain": ("void (anonymous namespace)::k_pn_splat<false>", "k_pn_splat<false>"), "vertex_density": ("k_pn_vertex_density",),
          "trim_face_mark": ("k_tr_face_mark",), "trim_vertex_count": ("k_tr_vertex_count",), "trim_vertex_scatter": ("k_tr_vertex_scatter",),
          "trim_face_scatter": ("k_tr_face_scatter",), "trim_scan": ("k_ct_scan", "k_ct_strided")}


def summarise(path):
    out = {g: dict(calls=0, total_us=0.0) for g in GROUPS}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for g, names in GROUPS.items():
                if any(n in row["Name"] for n in names):
                    out[g]["calls"] += int(row["Calls"])
                    out[g]["total_us"] += int(row["TotalDurationNs"]) / 1e3
    print(json.dumps(out))


def timed(torch, st, calls, fn):
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(round(e0.elapsed_time(e1), 3))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--depths", type=int, nargs="+", default=[8, 9])
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--solve-tol", type=float, default=1e-8)
    ap.add_argument("--trim-ratio", type=float, default=0.25)
    ap.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 run of this script: print the per-group sums and exit")
    a = ap.parse_args()
    if a.stats:
        return summarise(a.stats)
    import torch
    from multiviewstitch_amd import processor as P
    g = torch.Generator(device="cuda").manual_seed(7)
    d = torch.randn((a.points, 3), dtype=torch.float64, device="cuda", generator=g)
    d /= d.norm(dim=1, keepdim=True)
    ax = torch.tensor([1.0, 0.7, 0.5], dtype=torch.float64, device="cuda")
    q, _ = np.linalg.qr(np.random.default_rng(7).normal(size=(3, 3)))
    Rm = torch.as_tensor(q * np.sign(np.linalg.det(q)), dtype=torch.float64, device="cuda")
    nrm = d / ax
    nrm /= nrm.norm(dim=1, keepdim=True)
    pts, nrm = ((d * ax) @ Rm.T).contiguous(), (nrm @ Rm.T).contiguous()
    st = torch.cuda.current_stream()
    dprm = P.poisson_density_params(flags=P.WEIGHT_NORMALS)
    rows = []
    for D in a.depths:
        prm = P.poisson_params(depth_min=D, depth_max=D, solve_tol=a.solve_tol)
        v, f, info = P.RunPoisson(pts, nrm, prm, stream=st.cuda_stream)                # warm-up; sizes the outputs
        cap = (len(v), len(f))
        plain = timed(torch, st, a.calls, lambda: P.RunPoisson(pts, nrm, prm, stream=st.cuda_stream, capacity=cap))
        del v, f
        v, f, dens, dinfo = P.RunPoissonDensity(pts, nrm, prm, dprm, stream=st.cuda_stream)
        cap = (len(v), len(f))
        dense = timed(torch, st, a.calls, lambda: P.RunPoissonDensity(pts, nrm, prm, dprm, stream=st.cuda_stream, capacity=cap))
        row = dict(depth=info["depth"], cycles_plain=info["cycles"], cycles_weighted=dinfo["cycles"], vertices=len(v), faces=len(f),
                   density_depth=dinfo["density_depth"], mean_density=dinfo["mean_density"], min_point_density=dinfo["min_point_density"],
                   max_point_density=dinfo["max_point_density"], n_clamped=dinfo["n_clamped"], plain_ms=plain, plain_ms_best=min(plain),
                   plain_ms_spread=round(max(plain) - min(plain), 3), density_ms=dense, density_ms_best=min(dense),
                   density_ms_spread=round(max(dense) - min(dense), 3))
        if D == max(a.depths):
            thr = a.trim_ratio * dinfo["mean_density"]
            tv, tf = P.TrimByValue(v, f, dens, thr, stream=st.cuda_stream)             # warm-up
            trim = timed(torch, st, a.calls, lambda: P.TrimByValue(v, f, dens, thr, stream=st.cuda_stream))
            row.update(trim_ms=trim, trim_ms_best=min(trim), trim_kept_vertices=len(tv), trim_kept_faces=len(tf))
            del tv, tf
        rows.append(row)
        del v, f, dens
    print(json.dumps(dict(points=a.points, solve_tol=a.solve_tol, trim_ratio=a.trim_ratio, runs=rows)))


if __name__ == "__main__":
    main()
