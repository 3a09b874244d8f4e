"""First timing of GeometryRec::RunPoisson on the GPU (csrc/poisson.hip) at scan scale: 2 M oriented points sampled on a rotated ellipsoid
(semi-axes 1, 0.7, 0.5), resident in HBM, through mvs_poisson_reconstruct_dev at depth 8 and depth 9 (depth_min = depth_max).  Wall time
of the call from HIP events on its stream (warm: a first call sizes the outputs), V-cycles used, and the box's device-to-device copy
ceiling measured as bench.py --full measures it.  Per-kernel times come from running this script under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o poisson -- python scripts/bench_poisson.py --depths 9 --calls 1` (alone, no counters in the
same run); `python scripts/bench_poisson.py --stats <dir>/.../poisson_kernel_stats.csv --depth 9 --copy-gbps <ceiling>` then groups them
and gives the smoother's achieved bytes per second — 24 bytes per interior node and sweep: chi read once, b read, the result written —
against the ceiling.  No time is a pass criterion.  Prints one JSON line."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"cube_depth": ("k_pn_bbox", "k_pn_occupy", "k_pn_popcount"), "splat": ("k_pn_splat<false>", "k_pn_splat<true>"), "rhs": ("k_pn_rhs",),
          "smooth": ("k_mg_smooth<(anonymous namespace)::MgPlain>",), "residual": ("k_mg_residual<(anonymous namespace)::MgPlain>",),
          "restrict": ("k_mg_restrict",), "prolong": ("k_mg_prolong",), "coarse_levels": ("k_mg_coarse<(anonymous namespace)::MgPlain>",), "fold": ("k_pn_fold",), "iso": ("k_pn_iso",), "cube_mask": ("k_pn_cubemask",),
          "edge_count": ("k_pn_edge_count",), "vertex_scatter": ("k_pn_vertex_scatter",), "face_count": ("k_pn_face_count",),
          "face_scatter": ("k_pn_face_scatter",), "scan": ("k_ct_scan", "k_ct_strided")}


def summarise(path, depth, copy_gbps):
    out = {g: dict(calls=0, total_us=0.0) for g in GROUPS}
    smooth = []
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for g, names in GROUPS.items():
                if any(n + "(" in row["Name"] or row["Name"].startswith(n) for n in names):
                    out[g]["calls"] += int(row["Calls"])
                    out[g]["total_us"] += int(row["TotalDurationNs"]) / 1e3
                    if g == "smooth":
                        smooth.append(row)
    out["all_kernels_us"] = sum(v["total_us"] for v in out.values())
    if depth and out["smooth"]["calls"]:
        # the sweeps of the finest level dominate: a V(2,2) cycle runs 4 on every level above 33^3, each level an eighth of the one above
        G = 2 ** depth
        share = sum((2 ** l - 1) ** 3 for l in range(6, depth + 1))
        bytes_all = 24.0 * share * out["smooth"]["calls"] / max(1, depth - 5)
        gbps = bytes_all / (out["smooth"]["total_us"] * 1e-6) / 1e9
        out["smooth_GBps"] = round(gbps, 1)
        out["smooth_interior_nodes_finest"] = (G - 1) ** 3
        if copy_gbps:
            out["copy_ceiling_GBps"] = copy_gbps
            out["smooth_frac_of_copy_ceiling"] = round(gbps / copy_gbps, 4)
    print(json.dumps(out))


def copy_ceiling(torch):
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
    return 10 * 2 * a.numel() * 8 / (1e-3 * e0.elapsed_time(e1)) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--depths", type=int, nargs="+", default=[8, 9])
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--solve-tol", type=float, default=1e-8)
    ap.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 run of this script: print the per-group sums and exit")
    ap.add_argument("--depth", type=int, default=0, help="with --stats: the depth that run used")
    ap.add_argument("--copy-gbps", type=float, default=0.0, help="with --stats: the copy ceiling a plain run reported")
    a = ap.parse_args()
    if a.stats:
        return summarise(a.stats, a.depth, a.copy_gbps)
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
    rows = []
    for D in a.depths:
        prm = P.poisson_params(depth_min=D, depth_max=D, solve_tol=a.solve_tol)
        v, f, info = P.RunPoisson(pts, nrm, prm, stream=st.cuda_stream)                # warm-up; sizes the outputs
        cap = (len(v), len(f))
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            P.RunPoisson(pts, nrm, prm, stream=st.cuda_stream, capacity=cap)
            e1.record(st)
            e1.synchronize()
            ms.append(round(e0.elapsed_time(e1), 3))
        vol = float((v[f[:, 0].long()] * torch.cross(v[f[:, 1].long()], v[f[:, 2].long()], dim=1)).sum() / 6.0)
        rows.append(dict(depth=info["depth"], grid=2 ** info["depth"] + 1, cycles=info["cycles"], rel_residual=info["rel_residual"], vertices=len(v),
                         faces=len(f), volume=vol, volume_exact=4.0 / 3.0 * np.pi * 0.35, call_ms=ms, call_ms_best=min(ms)))
        del v, f
    print(json.dumps(dict(points=a.points, solve_tol=a.solve_tol, copy_ceiling_GBps=round(copy_ceiling(torch), 1), runs=rows)))


if __name__ == "__main__":
    main()
