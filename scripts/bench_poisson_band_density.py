"""Timing of mvs_poisson_reconstruct_band_density_dev (csrc/poisson_band.hip, rules 32-35) beside mvs_poisson_reconstruct_band_dev, in one
process, on the scene of scripts/bench_poisson_band.py — oriented points on a rotated ellipsoid (semi-axes 1, 0.7, 0.5), resident in
HBM — resampled 4 : 1 across the plane x = 0 of the unit sphere the points come from: 2 M points, 1.6 M on one side and 0.4 M on the
other.  At every depth (9 and 10, from base_depth 8 with band 2) three calls: the band call, the new call with flags = 0 and the new
call with MVS_POISSON_WEIGHT_NORMALS.  Wall time of each from HIP events on its stream (warm: a first call sizes the outputs), the
iterations of every level, the peak scratch bytes and the density info.  The comparison is against the band call of the same run; no
time or ratio is a pass criterion.  Prints one JSON line; --md writes the table of it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(out):
    rows = ["| depth | call | ms (best of %d) | against the band call | iterations per level | scratch MB | V | n_clamped |" % out["calls"],
            "|---|---|---|---|---|---|---|---|"]
    for r in out["rows"]:
        if "error" in r:
            rows.append(f"| {r['depth']} | {r['call']} | failed: {r['error']} | | | | | |")
            continue
        its = ", ".join(f"{l}: {v}" for l, v in sorted(r["iterations"].items()))
        rows.append(f"| {r['depth']} | {r['call']} | {r['call_ms_best']:.1f} | {r['against_band']:.3f} x | {its} | {r['scratch_bytes'] / 1e6:.0f} | {r['vertices']} | "
                    f"{r.get('n_clamped', '')} |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--depths", type=int, nargs="+", default=[9, 10])
    ap.add_argument("--base-depth", type=int, default=8)
    ap.add_argument("--band", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
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

    out = dict(points=a.points, solve_tol=a.solve_tol, base_depth=a.base_depth, band=a.band, calls=a.calls, rows=[])
    bprm = P.poisson_band_params(base_depth=a.base_depth, band=a.band)
    for D in a.depths:
        prm = P.poisson_params(depth_min=D, depth_max=D, solve_tol=a.solve_tol)
        band_ms = None
        for call, dprm in (("band", None), ("band_density flags 0", P.poisson_density_params()),
                           ("band_density weighted", P.poisson_density_params(flags=P.WEIGHT_NORMALS))):
            row = dict(depth=D, call=call)
            try:
                if dprm is None:
                    run = lambda cap=None: P.RunPoissonBand(pts, nrm, prm, bprm, stream=st.cuda_stream, capacity=cap)
                else:
                    run = lambda cap=None, dprm=dprm: P.RunPoissonBandDensity(pts, nrm, prm, bprm, dprm, stream=st.cuda_stream, capacity=cap)
                first = run()
                ms = timed(run, first)
                info, binfo = (first[2], first[3]) if dprm is None else (first[3], first[4])
                if dprm is None:
                    band_ms = min(ms)
                else:
                    row.update(density_depth=first[5]["density_depth"], mean_density=first[5]["mean_density"], n_clamped=first[5]["n_clamped"])
                lv = range(binfo["base_depth"] + 1, info["depth"] + 1)
                row.update(depth=info["depth"], base_cycles=info["cycles"], vertices=len(first[0]), faces=len(first[1]), call_ms=ms, call_ms_best=min(ms),
                           against_band=min(ms) / band_ms if band_ms else None, iterations={l: binfo["iterations"][l] for l in lv},
                           free_nodes={l: binfo["n_free"][l] for l in lv}, n_open_edges=binfo["n_open_edges"], scratch_bytes=binfo["scratch_bytes"])
                del first
            except L.MvsError as e:                                           # a level that does not converge or does not fit: say so
                row.update(error=str(e))
            out["rows"].append(row)
    print(json.dumps(out))
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(table(out))


if __name__ == "__main__":
    main()
