"""Timing of the band-refined levels of the Poisson stage (csrc/poisson_band.hip, rules 24-31) beside the dense grid, in one process, on
the scene of scripts/bench_poisson.py: 2 M oriented points on a rotated ellipsoid (semi-axes 1, 0.7, 0.5), resident in HBM.  Three
calls: mvs_poisson_reconstruct_dev at depth_min = depth_max = 9 (the dense grid), mvs_poisson_reconstruct_band_dev at depth 9 and at
depth 10, both from base_depth 8 with band 2.  Wall time of each call from HIP events on its stream (warm: a first call sizes the
outputs); for the band calls the active blocks, the free nodes and the iterations of every level and the peak scratch bytes.  No time
or ratio is a pass criterion.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--depths", type=int, nargs="+", default=[9, 10], help="depths of the band calls")
    ap.add_argument("--dense-depth", type=int, default=9, help="depth of the dense call; 0: none")
    ap.add_argument("--base-depth", type=int, default=8)
    ap.add_argument("--band", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--solve-tol", type=float, default=1e-8)
    a = ap.parse_args()
    import torch
    from multiviewstitch_amd import _lib as L, processor as P
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

    def volume(v, f):
        return float((v[f[:, 0].long()] * torch.cross(v[f[:, 1].long()], v[f[:, 2].long()], dim=1)).sum() / 6.0)

    out = dict(points=a.points, solve_tol=a.solve_tol, base_depth=a.base_depth, band=a.band, volume_exact=4.0 / 3.0 * np.pi * 0.35)
    if a.dense_depth:
        prm = P.poisson_params(depth_min=a.dense_depth, depth_max=a.dense_depth, solve_tol=a.solve_tol)
        first = P.RunPoisson(pts, nrm, prm, stream=st.cuda_stream)
        ms = timed(lambda cap: P.RunPoisson(pts, nrm, prm, stream=st.cuda_stream, capacity=cap), first)
        v, f, info = first
        nn = (2 ** info["depth"] + 1) ** 3
        below = sum(3 * (2 ** l + 1) ** 3 for l in range(1, info["depth"]))
        out["dense"] = dict(depth=info["depth"], cycles=info["cycles"], rel_residual=info["rel_residual"], vertices=len(v), faces=len(f), volume=volume(v, f),
                            field_bytes=32 * nn + 8 * below, call_ms=ms, call_ms_best=min(ms))
        del first, v, f
    out["band"] = []
    bprm = P.poisson_band_params(base_depth=a.base_depth, band=a.band)
    for D in a.depths:
        prm = P.poisson_params(depth_min=D, depth_max=D, solve_tol=a.solve_tol)
        row = dict(depth=D)
        try:
            first = P.RunPoissonBand(pts, nrm, prm, bprm, stream=st.cuda_stream)
            ms = timed(lambda cap: P.RunPoissonBand(pts, nrm, prm, bprm, stream=st.cuda_stream, capacity=cap), first)
            v, f, info, binfo = first
            row.update(depth=info["depth"], base_cycles=info["cycles"], base_rel_residual=info["rel_residual"], vertices=len(v), faces=len(f),
                       volume=volume(v, f), call_ms=ms, call_ms_best=min(ms))
            del first, v, f
        except L.MvsError as e:                                               # a level that does not converge or does not fit: say so, with the numbers
            binfo = getattr(e, "band_info", None)
            row.update(error=str(e))
        if binfo:
            lv = range(binfo["base_depth"] + 1, D + 1)
            row.update(levels={l: dict(active_blocks=binfo["n_active_blocks"][l], free_nodes=binfo["n_free"][l], iterations=binfo["iterations"][l],
                                       rel_residual=binfo["rel_residual"][l]) for l in lv},
                       n_open_edges=binfo["n_open_edges"], scratch_bytes=binfo["scratch_bytes"], failed_level=binfo["failed_level"])
        out["band"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
