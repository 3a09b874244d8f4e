"""First timing of the depth recovery on the GPU (csrc/depth_recover.hip) at scan scale: 8 sequences x 16 cameras of 640 x 480, images
resident in HBM, default parameters (N = 7, 128 levels, 5 frames in the window, min_refs 2, peak 0.9, substep), through
mvs_recover_depth_maps_dev, warm.  The frames are those of scripts/bench_refine.py (scene.make_sequence's surface coloured by a smooth 3-D
texture); beside the sweep the same run times mvs_refine_depth_maps_dev on the same frames and that script's rasters.

The script is a driver: every step that uses the GPU is a child process under its own time limit, and a step that fails or runs out of
time ends the run.
  gpu    the _dev call between HIP events on its stream (--calls of them after a warm-up call), two runs compared byte for byte; the
         refinement likewise; for both the time per (pixel x level x reference): the pixels that can have a cost (the interior for the
         sweep, the candidates for the refinement), every level or hypothesis, every reference frame of the pixel's window
  numpy  the numpy restatement tests/ref_depth_recover.py for a band of --numpy-rows rows of ONE frame of the same input on the CPU, the
         time scaled to the frame's interior rows (stated as scaled), and how many pixels of the band differ from the GPU's (level, sum,
         cnt, out); at this size no margin is checked, so a difference is reported, not asserted
It prints one JSON line and, with --md, writes the table of profiles/r31/recover.md.  No time is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LIMITS = {"gpu": 420, "numpy": 420}                                       # seconds per step


def _flat(cameras, stacks):
    import torch
    from multiviewstitch_amd import _lib as L
    off, cams = L.seq_cams(cameras)
    return off, cams, torch.cat([s.reshape(-1) for s in stacks]).contiguous()


def _timed(st, calls, fn):
    import torch
    fn()                                                                  # warm-up
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def step_gpu(a):
    import torch
    from bench_refine import build
    from multiviewstitch_amd import _lib as L, processor as P
    cameras, imgs, depths, rprm = build(a)
    prm = P.depth_recover_params()
    st = torch.cuda.current_stream()
    off, cams, fimg = _flat(cameras, imgs)
    _, _, fdep = _flat(cameras, depths)
    n, px = len(cameras), int(fdep.numel())
    out = [torch.empty(px, dtype=torch.float32, device="cuda") for _ in range(2)]
    lv, sm, cnt = (torch.empty(px, dtype=dt, device="cuda") for dt in (torch.int16, torch.int32, torch.uint8))
    rout, rk, rsm, rcnt = (torch.empty(px, dtype=dt, device="cuda") for dt in (torch.float32, torch.int8, torch.int32, torch.uint8))
    lib = L.lib()

    def sweep(o=0):
        L.check(lib.mvs_recover_depth_maps_dev(n, L.ptr(off), cams, L.ptr(fimg), C.byref(prm), L.ptr(out[o]), L.ptr(lv), L.ptr(sm), L.ptr(cnt),
                                               L.ptr(st.cuda_stream)))

    def refine():
        L.check(lib.mvs_refine_depth_maps_dev(n, L.ptr(off), cams, L.ptr(fimg), L.ptr(fdep), C.byref(rprm), L.ptr(rout), L.ptr(rk), L.ptr(rsm), L.ptr(rcnt),
                                              L.ptr(st.cuda_stream)))

    ms = _timed(st, a.calls, sweep)
    sweep(1)
    same = bool(torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)))
    rms = _timed(st, a.calls, refine)
    N, half = prm.ssd_win, prm.ref_frm_count // 2
    interior = max(0, a.w - 2 * N) * max(0, a.h - 2 * N)
    refs = [min(f + half, a.frames - 1) - max(f - half, 0) for f in range(a.frames)]
    work = a.seqs * interior * prm.levels * sum(refs)                     # pixel x level x reference of the sweep
    rcand = (rsm >= 0).reshape(a.seqs, a.frames, -1).sum(dim=(0, 2)).cpu().numpy()
    rwork = int((2 * rprm.steps + 1) * sum(int(c) * r for c, r in zip(rcand, refs)))
    truth = torch.cat([d.reshape(-1) for d in depths])                    # the refinement's inputs lie within 4 % of the true values
    acc = lv >= 0
    near = (torch.abs(out[0][acc].double() / truth[acc].double().clamp_min(1e-30) - 1.0) <= 0.05) & (truth[acc] > 0)
    return dict(step="gpu", seqs=a.seqs, frames=a.frames, w=a.w, h=a.h, ssd_win=N, levels=prm.levels, ref_frm_count=prm.ref_frm_count,
                min_refs=prm.min_refs, peak=prm.peak, pixels=px, interior_pixels=a.seqs * a.frames * interior,
                with_an_eligible_level=int((sm >= 0).sum()), accepted=int(acc.sum()), accepted_within_5pc_of_the_refinement_input=int(near.sum()),
                surface_pixels=int((truth > 0).sum()), call_ms=ms, call_ms_best=min(ms), runs_identical=same,
                pixel_level_references=work, ns_per_pixel_level_reference=min(ms) * 1e6 / work,
                refine_call_ms=rms, refine_call_ms_best=min(rms), refine_steps=rprm.steps, refine_pixel_level_references=rwork,
                refine_ns_per_pixel_level_reference=min(rms) * 1e6 / max(1, rwork),
                tiles=a.seqs * a.frames * (-(-a.w // 16)) * (-(-a.h // 16)))


def step_numpy(a):
    from bench_refine import build
    from multiviewstitch_amd import processor as P
    from tests import ref_depth_recover as R
    a.seqs = 1
    cameras, imgs, _, _ = build(a)
    prm = P.depth_recover_params()
    ((out, lv, sm, cnt),) = P.RecoverDepthMaps(cameras, imgs, prm, with_detail=True)
    f = a.frames // 2
    p = {k: getattr(prm, k) for k, _ in prm._fields_}
    G = R.grey(imgs[0].cpu().numpy())
    v0 = a.h // 2 - a.numpy_rows // 2
    only = np.zeros((a.h, a.w), bool)
    only[v0:v0 + a.numpy_rows] = True
    t0 = time.perf_counter()
    fr = R.recover_frame(cameras[0], G, f, p, R.Margins(), only=only)
    sec = time.perf_counter() - t0
    band = slice(v0, v0 + a.numpy_rows)
    differ = {key: int((got[f].cpu().numpy()[band] != fr[key][band]).sum()) for key, got in (("level", lv), ("sum", sm), ("cnt", cnt))}
    differ["out"] = int((out[f].cpu().numpy().view(np.uint32)[band] != fr["out"].view(np.uint32)[band]).sum())
    rows = a.h - 2 * prm.ssd_win
    return dict(step="numpy", frame=f, w=a.w, h=a.h, rows=a.numpy_rows, numpy_band_s=sec, numpy_one_frame_s_scaled=sec * rows / a.numpy_rows,
                accepted=int(fr["accepted"].sum()), pixels_that_differ=differ)


def write_md(path, res):
    g, n = res["gpu"], res.get("numpy")
    best, rbest = g["call_ms_best"], g["refine_call_ms_best"]
    lines = ["| quantity | value |", "|---|---|",
             f"| shape | {g['seqs']} sequences x {g['frames']} cameras x {g['w']} x {g['h']}, N = {g['ssd_win']}, L = {g['levels']}, window of "
             f"{g['ref_frm_count']} frames, min_refs {g['min_refs']}, peak {g['peak']} |",
             f"| mvs_recover_depth_maps_dev, warm (HIP events, {len(g['call_ms'])} calls) | {', '.join(f'{m:.2f}' for m in g['call_ms'])} ms; best {best:.2f} ms |",
             f"| per frame | {best / (g['seqs'] * g['frames']):.3f} ms |",
             f"| pixels / interior / with an eligible level / accepted | {g['pixels']} / {g['interior_pixels']} / {g['with_an_eligible_level']} / {g['accepted']} |",
             f"| accepted within 5 % of the rasters the refinement was given / pixels on the surface | {g['accepted_within_5pc_of_the_refinement_input']} / {g['surface_pixels']} |",
             f"| pixel x level x reference | {g['pixel_level_references']:.3e}; {g['ns_per_pixel_level_reference'] * 1e3:.3f} ps each at the best call |",
             f"| workgroups of the sweep | {g['tiles']} of 256 threads |",
             f"| two calls give the same bytes | {g['runs_identical']} |",
             f"| mvs_refine_depth_maps_dev on the same frames, same run (K = {g['refine_steps']}) | {', '.join(f'{m:.2f}' for m in g['refine_call_ms'])} ms; best {rbest:.2f} ms |",
             f"| its candidate x hypothesis x reference | {g['refine_pixel_level_references']:.3e}; {g['refine_ns_per_pixel_level_reference'] * 1e3:.3f} ps each at the best call |"]
    if n:
        lines += [f"| numpy restatement, {n['rows']} rows of ONE frame ({n['w']} x {n['h']}, CPU) | {n['numpy_band_s']:.1f} s; scaled to the frame's interior rows "
                  f"{n['numpy_one_frame_s_scaled']:.0f} s |",
                  f"| pixels of that band that differ from the GPU (level / sum / cnt / out bits) | {n['pixels_that_differ']['level']} / {n['pixels_that_differ']['sum']} / "
                  f"{n['pixels_that_differ']['cnt']} / {n['pixels_that_differ']['out']} |"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--numpy-rows", type=int, default=8)
    ap.add_argument("--step", choices=("gpu", "numpy"), help="run one step in this process (the driver starts these)")
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--md", help="write the table to this file")
    a = ap.parse_args()
    if a.step:
        print(json.dumps((step_gpu if a.step == "gpu" else step_numpy)(a)))
        return 0
    res = {}
    for step in ("gpu",) + (() if a.skip_numpy else ("numpy",)):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--seqs", str(a.seqs), "--frames", str(a.frames), "--w", str(a.w), "--h", str(a.h),
               "--calls", str(a.calls), "--numpy-rows", str(a.numpy_rows)]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[step])
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(res, failed=step, why=f"no result within {LIMITS[step]} s")))
            return 1
        if run.returncode != 0:
            print(json.dumps(dict(res, failed=step, rc=run.returncode, stderr=run.stderr[-2000:])))
            return 1
        res[step] = json.loads(run.stdout.strip().splitlines()[-1])
    if a.md:
        write_md(a.md, res)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
