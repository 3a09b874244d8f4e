"""Timing of mvs_poisson_reconstruct_band_screened_dev (csrc/poisson_band.hip, rules 36-41) beside
mvs_poisson_reconstruct_band_density_dev, in one process, on the scene of scripts/bench_poisson_band_density.py: 2 M oriented points on
a rotated ellipsoid (semi-axes 1, 0.7, 0.5), resident in HBM, resampled 4 : 1 across the plane x = 0 of the unit sphere the points
come from.  At every depth (9 and 10, from base_depth 8 with band 2), unweighted and with MVS_POISSON_WEIGHT_NORMALS, two calls: the
band-density call and the new call at alpha = 4.  Wall time of each from HIP events on its stream (warm: a first call sizes the
outputs; three calls, all listed, the median and the best named), the iterations and the stencil rows of every level, the cycles of the
two base solves, the peak scratch bytes, the open edges, and the radial error of the mesh against the analytic surface: a vertex v
maps back to u = (R^T v) / axes on the unit sphere, and |u| - 1 is its error there (rms and maximum; dimensionless, 1 / 2^depth * 2.2
is about one cell).  The comparison is against the band-density call of the same run; no time or ratio is a pass criterion.  Prints
one JSON line; --md writes the table of it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(out):
    rows = ["| depth | call | ms (median of %d) | best | against band_density | iterations per level | rows per level | base cycles | scratch MB | V | open edges "
            "| radial rms | radial max |" % out["calls"], "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["rows"]:
        if "error" in r:
            rows.append(f"| {r['depth']} | {r['call']} | failed: {r['error']} | | | | | | | | | | |")
            continue
        its = ", ".join(f"{l}: {v}" for l, v in sorted(r["iterations"].items()))
        nrows = ", ".join(f"{l}: {v}" for l, v in sorted(r.get("rows", {}).items()))
        against = f"{r['against_band_density']:.3f} x" if r.get("against_band_density") else ""
        rows.append(f"| {r['depth']} | {r['call']} | {r['call_ms_median']:.1f} | {r['call_ms_best']:.1f} | {against} | {its} | {nrows} | {r['base_cycles']} | "
                    f"{r['scratch_bytes'] / 1e6:.0f} | {r['vertices']} | {r['n_open_edges']} | {r['radial_rms']:.3e} | {r['radial_max']:.3e} |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--depths", type=int, nargs="+", default=[9, 10])
    ap.add_argument("--base-depth", type=int, default=8)
    ap.add_argument("--band", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--alpha", type=float, default=4.0)
    ap.add_argument("--solve-tol", type=float, default=1e-8)
    ap.add_argument("--md", default=None, help="write the table here")
    a = ap.parse_args()
    import torch
    from multiviewstitch_amd import _lib as L, processor as P
    g = torch.Generator(device="cuda").manual_seed(7)
    d = torch.randn((2 * a.points, 3), dtype=torch.float64, device="cuda", generator=g)
    d /= d.norm(dim=1, keepdim=True)
    dense, sparse = d[d[:, 0] > 0.0][:a.points * 4 // 5], d[d[:, 0] <= 0.0][:a.points // 5]
    d = torch.cat([dense, sparse])
    assert len(d) == a.points, "too few directions on one side"
    ax = torch.tensor([1.0, 0.7, 0.5], dtype=torch.float64, device="cuda")
    q, _ = np.linalg.qr(np.random.default_rng(7).normal(size=(3, 3)))
    Rm = torch.as_tensor(q * np.sign(np.linalg.det(q)), dtype=torch.float64, device="cuda")
    nrm = d / ax
    nrm /= nrm.norm(dim=1, keepdim=True)
    pts, nrm = ((d * ax) @ Rm.T).contiguous(), (nrm @ Rm.T).contiguous()
    st = torch.cuda.current_stream()

    def timed(run, first):
        cap = (len(first[0]), len(first[1]))
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            run(cap)
            e1.record(st)
            e1.synchronize()
            ms.append(round(e0.elapsed_time(e1), 3))
        return ms

    def radial(v):
        r = ((v @ Rm) / ax).norm(dim=1) - 1.0
        return float((r * r).mean().sqrt()), float(r.abs().max())

    out = dict(points=a.points, solve_tol=a.solve_tol, base_depth=a.base_depth, band=a.band, calls=a.calls, alpha=a.alpha, rows=[])
    bprm, sprm = P.poisson_band_params(base_depth=a.base_depth, band=a.band), P.poisson_screen_params(alpha=a.alpha)
    for D in a.depths:
        prm = P.poisson_params(depth_min=D, depth_max=D, solve_tol=a.solve_tol)
        for weight in (False, True):
            dprm = P.poisson_density_params(flags=P.WEIGHT_NORMALS if weight else 0)
            ref_ms = None
            for call in ("band_density", "band_screened"):
                row = dict(depth=D, call=call + (" weighted" if weight else " flags 0"))
                try:
                    if call == "band_density":
                        run = lambda cap=None: P.RunPoissonBandDensity(pts, nrm, prm, bprm, dprm, stream=st.cuda_stream, capacity=cap)
                    else:
                        run = lambda cap=None: P.RunPoissonBandScreened(pts, nrm, prm, bprm, dprm, sprm, stream=st.cuda_stream, capacity=cap)
                    first = run()
                    ms = timed(run, first)
                    info, binfo = first[3], first[4]
                    lv = range(binfo["base_depth"] + 1, info["depth"] + 1)
                    rms, rmax = radial(first[0])
                    row.update(depth=info["depth"], base_cycles=info["cycles"], vertices=len(first[0]), faces=len(first[1]), call_ms=ms,
                               call_ms_median=statistics.median(ms), call_ms_best=min(ms), iterations={l: binfo["iterations"][l] for l in lv},
                               free_nodes={l: binfo["n_free"][l] for l in lv}, n_open_edges=binfo["n_open_edges"], scratch_bytes=binfo["scratch_bytes"],
                               rel_residual={l: binfo["rel_residual"][l] for l in lv}, radial_rms=rms, radial_max=rmax, iso=info["iso"])
                    if call == "band_density":
                        ref_ms = statistics.median(ms)
                    else:
                        sinfo, bsinfo = first[6], first[7]
                        row.update(against_band_density=statistics.median(ms) / ref_ms if ref_ms else None, rows={l: bsinfo["active_nodes"][l] for l in lv},
                                   lambdas={l: bsinfo["lambda"][l] for l in lv}, targets={l: bsinfo["target"][l] for l in lv},
                                   base_screen_cycles=sinfo["screen_cycles"], base_lambda=sinfo["lambda"], base_rows=sinfo["active_nodes"])
                        row["base_cycles"] = f"{info['cycles']} + {sinfo['screen_cycles']}"
                    del first
                except L.MvsError as e:                                       # a level that does not converge or does not fit: say so
                    row.update(error=str(e))
                out["rows"].append(row)
    print(json.dumps(out))
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(table(out))


if __name__ == "__main__":
    main()
