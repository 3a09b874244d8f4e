"""Timing of the screened Poisson call (csrc/poisson.hip, rules 19-23 of include/mvs.h) with the set-up of scripts/bench_poisson_density.py:
2 M oriented points on a rotated ellipsoid (semi-axes 1, 0.7, 0.5), resident in HBM, depth 8 and depth 9 (depth_min = depth_max).  Per
depth, from HIP events on the call's stream, three calls after a warm-up each: mvs_poisson_reconstruct_density_dev — the code of that
entry is the parent commit's, so this is the parent's time on the same box in the same run — and mvs_poisson_reconstruct_screened_dev at
the default alpha; their spread (max - min over the calls) is the run-to-run spread the comparison has to respect.  With them the cycles
of both solves and the nodes with a stencil row on every level (counted here with torch from the points, not read from the library).
`--diagonals` runs the three Jacobi diagonals of mvs_test_poisson_screened on the small scenes of tests/poisson_screened_scenes.py and
prints the cycles each needs at solve_tol 1e-12 (or the residual it reached in --max-cycles).  Per-kernel times come from running this
script under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o screened -- python scripts/bench_poisson_screened.py
--depths 9 --calls 1` (alone, no counters in the same run); `--stats <dir>/.../screened_kernel_stats.csv --bench-json <that run's JSON
line in a file>` then groups the kernels and computes the smoothers' achieved bandwidth beside the 4.08 TB/s of profiles/r16/poisson.md.
The diagnostics build of the library (`make EXPERIMENTS=1`) reads MVS_SC_SMOOTH_BY_ROWS: 1 runs the smoother as the plain kernel plus
a pass over the rows instead of the fused kernel.  No time is a pass criterion.  Prints one JSON line."""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN, SCREENED = "<(anonymous namespace)::MgPlain", "<(anonymous namespace)::MgScreened"      # the operator, first template argument of a multigrid kernel
GROUPS = {"smooth_plain": ("k_mg_smooth" + PLAIN,), "smooth_screened": ("k_mg_smooth" + SCREENED,), "smooth_rows": ("k_sc_smooth_rows",),
          "residual_plain": ("k_mg_residual" + PLAIN,), "residual_screened": ("k_mg_residual" + SCREENED,), "coarse_plain": ("k_mg_coarse" + PLAIN,),
          "coarse_screened": ("k_mg_coarse" + SCREENED,),
          "restrict": ("k_mg_restrict",), "prolong": ("k_mg_prolong",), "stencil_flag": ("k_sc_flag(",), "stencil_number": ("k_sc_count", "k_sc_number"),
          "stencil_splat": ("k_sc_splat",), "stencil_coarsen": ("k_sc_flag_coarse", "k_sc_coarsen"), "stencil_convert": ("k_sc_convert",), "screen_rhs": ("k_sc_rhs",), "occupy": ("k_pn_occupy", "k_pn_popcount")}


COARSE = 5                               # csrc/poisson.hip, PN_COARSE: the levels above it are launched one kernel a sweep


def summarise(path, bench_json):
    """the per-group sums and, with the JSON line of a run of this script, the smoothers' achieved bandwidth at its deepest depth D: a
    sweep of the launched levels COARSE + 1 .. D is one launch per level.  `min`: 24 bytes per interior node (chi read once, b read, the
    result written), the accounting of profiles/r16/poisson.md (4.08 TB/s there).  `moved`, for the fused smoother: 4 more bytes per node
    for the row number and 224 bytes per row."""
    out = {g: dict(calls=0, total_us=0.0) for g in GROUPS}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for g, names in GROUPS.items():
                if any(n in row["Name"] for n in names):
                    out[g]["calls"] += int(row["Calls"])
                    out[g]["total_us"] += int(row["TotalDurationNs"]) / 1e3
    if bench_json:
        with open(bench_json) as fh:
            run = max(json.loads(fh.readline())["runs"], key=lambda r: r["depth"])
        D, levels = run["depth"], range(COARSE + 1, run["depth"] + 1)
        interior = sum((2 ** l - 1) ** 3 for l in levels)
        rows = sum(run["rows_per_level"][str(l)] for l in levels)
        for g, per_sweep in (("smooth_plain", dict(min=24 * interior)), ("smooth_screened", dict(min=24 * interior, moved=28 * interior + 224 * rows))):
            if out[g]["calls"]:
                sweeps = out[g]["calls"] / len(levels)
                out[g].update(depth=D, us_per_launch=round(out[g]["total_us"] / out[g]["calls"], 1),
                              **{f"tb_per_s_{k}": round(v * sweeps / (out[g]["total_us"] * 1e-6) / 1e12, 3) for k, v in per_sweep.items()})
        if out["smooth_rows"]["calls"]:
            r, pl = out["smooth_rows"], out["smooth_plain"]                    # a screened sweep of a level: one plain launch, one pass over the rows
            us = r["total_us"] + r["calls"] * pl["total_us"] / pl["calls"]
            r.update(us_per_launch=round(r["total_us"] / r["calls"], 1), rows_per_sweep=rows, us_per_launch_with_plain=round(us / r["calls"], 1),
                     tb_per_s_min_with_plain=round(24 * interior * (r["calls"] / len(levels)) / (us * 1e-6) / 1e12, 3))
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


def rows_per_level(torch, pts, origin, h, D):
    """the nodes a point touches on every level l = D .. 1: the distinct corners of the points' cells"""
    out = {}
    o = torch.as_tensor(origin, dtype=torch.float64, device=pts.device)
    for l in range(D, 0, -1):
        G = 2 ** l
        i0 = torch.clamp(torch.floor((pts - o) / (h * 2 ** (D - l))), 0, G - 1).to(torch.int64)
        ids = [((i0[:, 2] + (c >> 2 & 1)) * (G + 1) + i0[:, 1] + (c >> 1 & 1)) * (G + 1) + i0[:, 0] + (c & 1) for c in range(8)]
        out[l] = int(torch.unique(torch.cat(ids)).numel())
    return out


def diagonals(max_cycles):
    from multiviewstitch_amd import _lib as L, processor as P
    from tests import poisson_screened_scenes as SC
    rows = []
    for name in SC.NAMES:
        pts, nrm, prm, dprm, weight, alpha = SC.scene(name)
        nn = (2 ** SC.DEPTHS[name] + 1) ** 3
        row = dict(scene=name, alpha=alpha)
        for mode, label in ((0, "half_row_sum"), (1, "plain"), (2, "row_sum")):
            st, f, chi0, chi = np.zeros((nn, 27), np.int64), np.zeros(nn), np.zeros(nn), np.zeros(nn)
            ci, di, si = L.CPoissonInfo(), L.CPoissonDensityInfo(), L.CPoissonScreenInfo()
            p = P.poisson_params(**dict(prm, solve_tol=SC.TOL, max_cycles=max_cycles))
            dp, sp = P.poisson_density_params(flags=P.WEIGHT_NORMALS if weight else 0, **dprm), P.poisson_screen_params(alpha=alpha)
            rc = L.lib().mvs_test_poisson_screened(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(p), C.byref(dp), C.byref(sp), C.byref(ci), C.byref(di),
                                                   C.byref(si), L.ptr(st), L.ptr(f), L.ptr(chi0), L.ptr(chi), nn, mode)
            row[label] = dict(rc=rc, cycles=si.cycles, rel_residual=si.rel_residual)
            row["first_solve_cycles"] = ci.cycles
        rows.append(row)
    print(json.dumps(dict(solve_tol=SC.TOL, max_cycles=max_cycles, diagonals=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--depths", type=int, nargs="+", default=[8, 9])
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--solve-tol", type=float, default=1e-8)
    ap.add_argument("--alpha", type=float, default=4.0)
    ap.add_argument("--diagonals", action="store_true", help="cycles of the three Jacobi diagonals on the small test scenes, then exit")
    ap.add_argument("--max-cycles", type=int, default=300)
    ap.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 run of this script: print the per-group sums and exit")
    ap.add_argument("--bench-json", help="with --stats: the JSON line that run printed, for the smoothers' bandwidth")
    a = ap.parse_args()
    if a.stats:
        return summarise(a.stats, a.bench_json)
    if a.diagonals:
        return diagonals(a.max_cycles)
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
    dprm, sprm = P.poisson_density_params(), P.poisson_screen_params(alpha=a.alpha)
    rows = []
    for D in a.depths:
        prm = P.poisson_params(depth_min=D, depth_max=D, solve_tol=a.solve_tol)
        v, f, dens, dinfo = P.RunPoissonDensity(pts, nrm, prm, dprm, stream=st.cuda_stream)          # warm-up; sizes the outputs
        cap = (len(v), len(f))
        dense = timed(torch, st, a.calls, lambda: P.RunPoissonDensity(pts, nrm, prm, dprm, stream=st.cuda_stream, capacity=cap))
        del v, f, dens
        v, f, dens, sinfo = P.RunPoissonScreened(pts, nrm, prm, dprm, sprm, stream=st.cuda_stream)
        cap = (len(v), len(f))
        per_level = rows_per_level(torch, pts, sinfo["origin"], sinfo["h"], sinfo["depth"])
        assert per_level[sinfo["depth"]] == sinfo["active_nodes"]                                  # the library's own count of the finest level
        scr = timed(torch, st, a.calls, lambda: P.RunPoissonScreened(pts, nrm, prm, dprm, sprm, stream=st.cuda_stream, capacity=cap))
        rows.append(dict(depth=sinfo["depth"], cycles_first=sinfo["cycles"], cycles_density_call=dinfo["cycles"], cycles_screened=sinfo["screen_cycles"],
                         rel_residual_screened=sinfo["screen_rel_residual"], lam=sinfo["lambda"], occupied=sinfo["occupied"],
                         active_nodes=sinfo["active_nodes"], rows_per_level=per_level,
                         nodes=(2 ** D + 1) ** 3, vertices=len(v), faces=len(f), density_ms=dense, density_ms_best=min(dense),
                         density_ms_spread=round(max(dense) - min(dense), 3), screened_ms=scr, screened_ms_best=min(scr),
                         screened_ms_spread=round(max(scr) - min(scr), 3), ratio_best=round(min(scr) / min(dense), 3)))
        del v, f, dens
    print(json.dumps(dict(points=a.points, solve_tol=a.solve_tol, alpha=a.alpha, runs=rows)))


if __name__ == "__main__":
    main()
