"""First timing of the aggregated depth recovery on the GPU (csrc/depth_sgm.hip) on the shape of profiles/r31/recover.md: 8 sequences x 16
cameras of 640 x 480, images resident in HBM, the default parameters of both structs (N = 7, 128 levels, 8 paths), through
mvs_recover_depth_maps_aggregated_dev, warm, between HIP events on the stream of the inputs — and, in the same process on the same
frames, mvs_recover_depth_maps_dev timed the same way.  The frames are those of scripts/bench_refine.py.

The script is a driver: the step that uses the GPU is a child process under its own time limit.  For the split of the call between its
kernels run the step itself under a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_recover_sgm.py --step gpu --calls 1
It prints one JSON line and, with --md, writes the table of profiles/r33/recover_sgm.md.  No time is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LIMIT = 540                                                               # seconds for the GPU step


def step_gpu(a):
    import torch
    from bench_recover import _flat, _timed
    from bench_refine import build
    from multiviewstitch_amd import _lib as L, processor as P
    cameras, imgs, depths, _ = build(a)
    prm, aprm = P.depth_recover_params(), P.depth_aggregate_params(paths=a.paths)
    st = torch.cuda.current_stream()
    off, cams, fimg = _flat(cameras, imgs)
    truth = torch.cat([d.reshape(-1) for d in depths])                    # within 4 % of the true values (bench_refine.build)
    n, px = len(cameras), int(truth.numel())
    out = {k: [torch.empty(px, dtype=torch.float32, device="cuda") for _ in range(2)] for k in ("plain", "agg")}
    lv = {k: torch.empty(px, dtype=torch.int16, device="cuda") for k in ("plain", "agg")}
    sm, cnt, ag = (torch.empty(px, dtype=dt, device="cuda") for dt in (torch.int32, torch.uint8, torch.int32))
    lib = L.lib()

    def plain(o=0):
        L.check(lib.mvs_recover_depth_maps_dev(n, L.ptr(off), cams, L.ptr(fimg), C.byref(prm), L.ptr(out["plain"][o]), L.ptr(lv["plain"]), L.ptr(sm),
                                               L.ptr(cnt), L.ptr(st.cuda_stream)))

    def agg(o=0):
        L.check(lib.mvs_recover_depth_maps_aggregated_dev(n, L.ptr(off), cams, L.ptr(fimg), C.byref(prm), C.byref(aprm), L.ptr(out["agg"][o]),
                                                          L.ptr(lv["agg"]), L.ptr(sm), L.ptr(cnt), L.ptr(ag), L.ptr(st.cuda_stream)))

    ms = {"agg": _timed(st, a.calls, agg), "plain": _timed(st, a.calls, plain)}
    ms["agg_again"] = _timed(st, a.calls, agg) if a.calls > 1 else []     # the spread between two windows of the same call
    agg(1)
    same = bool(torch.equal(out["agg"][0].view(torch.int32), out["agg"][1].view(torch.int32)))
    N, L_ = prm.ssd_win, prm.levels
    rect = max(0, a.w - 2 * N) * max(0, a.h - 2 * N)
    frames = a.seqs * a.frames
    counts = {}
    for k in ("plain", "agg"):
        acc = lv[k] >= 0
        near = (torch.abs(out[k][0][acc].double() / truth[acc].double().clamp_min(1e-30) - 1.0) <= 0.05) & (truth[acc] > 0)
        counts[k] = dict(accepted=int(acc.sum()), within_5pc=int(near.sum()), accepted_off_the_surface=int((truth[acc] <= 0).sum()))
    # bytes the rules need per frame: C written once; per direction C read and S read and written, but for the first direction, which only
    # writes S; the selection reads S
    vol = 2 * rect * L_
    need = vol + aprm.paths * 3 * vol - vol + vol
    return dict(step="gpu", seqs=a.seqs, frames=a.frames, w=a.w, h=a.h, ssd_win=N, levels=L_, paths=aprm.paths, p1=aprm.p1, p2=aprm.p2, cost_cap=aprm.cost_cap,
                pixels=px, rectangle_pixels=frames * rect, surface_pixels=int((truth > 0).sum()), counts=counts, call_ms=ms, runs_identical=same,
                volume_mb_per_frame=2 * vol / 2**20, frames_per_group=int(((aprm.max_volume_mb or L.SGM_VOLUME_MB) << 20) // max(1, 2 * vol)),
                volume_budget_mb=int(aprm.max_volume_mb or L.SGM_VOLUME_MB), volume_bytes_needed_per_frame=need,
                lines_per_frame={"rows": a.h - 2 * N, "columns": a.w - 2 * N, "each diagonal family": a.w + a.h - 4 * N - 1})


def write_md(path, g):
    ms, c = g["call_ms"], g["counts"]
    frames = g["seqs"] * g["frames"]
    best = {k: min(v) for k, v in ms.items() if v}
    row = lambda k: f"{', '.join(f'{m:.2f}' for m in ms[k])} ms; best {best[k]:.2f} ms; {best[k] / frames:.3f} ms per frame"
    lines = ["| quantity | value |", "|---|---|",
             f"| shape | {g['seqs']} sequences x {g['frames']} cameras x {g['w']} x {g['h']}, N = {g['ssd_win']}, L = {g['levels']}, paths {g['paths']}, p1 {g['p1']}, "
             f"p2 {g['p2']}, cost_cap {g['cost_cap']} |",
             f"| mvs_recover_depth_maps_aggregated_dev, warm (HIP events) | {row('agg')} |",
             f"| the same again after the plain sweep | {row('agg_again') if ms['agg_again'] else 'not run'} |",
             f"| mvs_recover_depth_maps_dev, same process, same frames | {row('plain')} |",
             f"| aggregation on top of the sweep, per frame (best - best) | {(best['agg'] - best['plain']) / frames:.3f} ms |",
             f"| volumes of one frame / frames per group at a budget of {g['volume_budget_mb']} MB | {g['volume_mb_per_frame']:.1f} MB / {g['frames_per_group']} |",
             f"| bytes of the volumes the rules move per frame | {g['volume_bytes_needed_per_frame'] / 1e9:.3f} GB |",
             f"| lines (waves) per frame | {g['lines_per_frame']} |",
             f"| rectangle pixels / pixels on the surface | {g['rectangle_pixels']} / {g['surface_pixels']} |",
             f"| plain: accepted / within 5 % of the truth / accepted off the surface | {c['plain']['accepted']} / {c['plain']['within_5pc']} / "
             f"{c['plain']['accepted_off_the_surface']} |",
             f"| aggregated: accepted / within 5 % of the truth / accepted off the surface | {c['agg']['accepted']} / {c['agg']['within_5pc']} / "
             f"{c['agg']['accepted_off_the_surface']} |",
             f"| two aggregated calls give the same bytes | {g['runs_identical']} |"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--step", choices=("gpu",), help="run the step in this process (the driver starts it)")
    ap.add_argument("--md", help="write the table to this file")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step_gpu(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu", "--seqs", str(a.seqs), "--frames", str(a.frames), "--w", str(a.w), "--h", str(a.h),
           "--calls", str(a.calls), "--paths", str(a.paths)]
    try:
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(failed="gpu", why=f"no result within {LIMIT} s")))
        return 1
    if run.returncode != 0:
        print(json.dumps(dict(failed="gpu", rc=run.returncode, stderr=run.stderr[-2000:])))
        return 1
    res = json.loads(run.stdout.strip().splitlines()[-1])
    if a.md:
        write_md(a.md, res)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
