"""First timing of the depth refinement on the GPU (csrc/depth_refine.hip) at scan scale: 8 sequences x 16 cameras of 640 x 480, images and
rasters resident in HBM, default parameters (N = 7, K = 8, 5 frames in the window), through mvs_refine_depth_maps_dev, warm.  The scene is
scene.make_sequence's surface (two of them, taken in turn), coloured by a smooth pseudo-random 3-D texture at every pixel's surface point;
the input rasters are the true ones times 1 + j * step with a seeded |j| <= K per 8 x 8 block.

The script is a driver: every step that uses the GPU is a child process under its own time limit, and a step that fails or runs out of
time ends the run.
  gpu    wall time of the call from HIP events on its stream (--calls of them after a warm-up call), two runs compared byte for byte
  numpy  the numpy restatement tests/ref_depth_refine.py for ONE frame of the same input on the CPU — the only other implementation there
         is — and how many pixels of that frame differ from the GPU's (k, sum, cnt, out); at this size no margin is checked, so a
         difference is reported, not asserted
It prints one JSON line and, with --md, writes the table of profiles/r22/refine.md.  Per-kernel times come from running the gpu step under
`rocprofv3 --kernel-trace --stats -d <dir> -o refine -- python scripts/bench_refine.py --step gpu` (alone, no counters in the same run).
No time is a pass criterion."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"gpu": 300, "numpy": 600}                                       # seconds per step


def texture_torch(X, seed):
    """a smooth colour at the points X [..., 3] (torch, float64) -> [..., 3] uint8; wavelengths of 6 to 20 pixels at this scale"""
    import torch
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        om = rng.normal(size=(10, 3))
        om *= (rng.uniform(50.0, 160.0, 10) / np.linalg.norm(om, axis=1))[:, None]
        ph, amp = rng.uniform(0, 2 * math.pi, 10), rng.uniform(0.5, 1.0, 10)
        val = sum(float(amp[i]) * torch.sin(X @ torch.as_tensor(om[i], device=X.device) + float(ph[i])) for i in range(10))
        out.append(127.5 + 110.0 * val / math.sqrt(float((amp * amp).sum()) * 2.0))
    return torch.clamp(torch.round(torch.stack(out, -1)), 0, 255).to(torch.uint8)


def build(a, dev="cuda"):
    """-> cameras[k], imgs[k] uint8 [n, h, w, 3], depths[k] float32 [n, h, w] (torch, on the GPU), params"""
    import torch
    from multiviewstitch_amd import processor as P, scene as S
    prm = P.depth_refine_params()
    step = prm.rel_range / prm.steps
    cameras, imgs, depths = [], [], []
    for k in range(a.seqs):
        if k < 2:                                                         # two surfaces, taken in turn (the ray caster is slow)
            cams, d = S.make_sequence(n_frames=a.frames, w=a.w, h=a.h, dyaw_deg=3.0, seed=77 + k, device=dev)
            d = torch.as_tensor(d, dtype=torch.float64, device=dev)
            im = torch.zeros((a.frames, a.h, a.w, 3), dtype=torch.uint8, device=dev)
            vv, uu = torch.meshgrid(torch.arange(a.h, dtype=torch.float64, device=dev), torch.arange(a.w, dtype=torch.float64, device=dev), indexing="ij")
            for f, c in enumerate(cams):
                hit = d[f] > 0
                z = 1.0 / torch.where(hit, d[f], torch.ones_like(d[f]))
                Rm, t = torch.as_tensor(np.asarray(c.R), device=dev), torch.as_tensor(np.asarray(c.t), device=dev)
                X = (torch.stack([(uu - c.cx) * z / c.fx, (vv - c.cy) * z / c.fy, z], -1) - t) @ Rm
                im[f] = torch.where(hit[..., None], texture_torch(X, 500 + k), torch.zeros_like(im[f]))
            rng = np.random.default_rng(900 + k)
            jb = rng.integers(-prm.steps, prm.steps + 1, size=(a.frames, -(-a.h // 8), -(-a.w // 8)))
            j = torch.as_tensor(np.repeat(np.repeat(jb, 8, 1), 8, 2)[:, :a.h, :a.w], device=dev)
            depths.append((d * (1.0 + j * step)).to(torch.float32).contiguous())
            imgs.append(im.contiguous())
        else:
            cams = cameras[k - 2]
            depths.append(depths[k - 2].clone())
            imgs.append(imgs[k - 2].clone())
        cameras.append(cams)
    return cameras, imgs, depths, prm


def step_gpu(a):
    import torch
    from multiviewstitch_amd import processor as P
    cameras, imgs, depths, prm = build(a)
    st = torch.cuda.current_stream()
    first = P.RefineAllDepthMaps(cameras, imgs, depths, prm, stream=st.cuda_stream, with_detail=True)          # warm-up
    ms = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        again = P.RefineAllDepthMaps(cameras, imgs, depths, prm, stream=st.cuda_stream, with_detail=True)
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for p, q in zip(first, again) for x, y in zip(p, q))
    cand = sum(int((r[2] >= 0).sum()) for r in again)
    acc = sum(int((r[1] != -128).sum()) for r in again)
    refs = sum(int(r[3].sum()) for r in again)
    px = a.seqs * a.frames * a.w * a.h
    # what rule 5 asks for at most, without the reuse of a window sum between hypotheses: every pixel with a winner, (2 K + 1) hypotheses,
    # the references of its frame's window, (2 N + 1)^2 differences each
    half = prm.ref_frm_count // 2
    diffs = (2 * prm.steps + 1) * (2 * prm.ssd_win + 1) ** 2 * sum(
        (min(f + half, len(c) - 1) - max(f - half, 0)) * int((r[2][f] >= 0).sum()) for c, r in zip(cameras, again) for f in range(len(c)))
    return dict(step="gpu", seqs=a.seqs, frames=a.frames, w=a.w, h=a.h, ssd_win=prm.ssd_win, steps=prm.steps,
                ref_frm_count=prm.ref_frm_count, pixels=px, pixels_with_a_winner=cand, accepted=acc, winner_references=refs, grey_differences_by_rule_5=diffs,
                call_ms=ms, call_ms_best=min(ms), runs_identical=bool(same), tiles=a.seqs * a.frames * (-(-a.w // 16)) * (-(-a.h // 16)))


def step_numpy(a):
    from multiviewstitch_amd import processor as P
    from tests import ref_depth_refine as R
    a.seqs = 1
    cameras, imgs, depths, prm = build(a)
    ((out, kk, sm, cnt),) = P.RefineAllDepthMaps(cameras, imgs, depths, prm, with_detail=True)
    f = a.frames // 2
    p = R.params(prm.dsp_min, prm.dsp_max, prm.rel_range, prm.ssd_err, prm.ssd_win, prm.ref_frm_count, prm.steps, prm.flags)
    G, d = R.grey(imgs[0].cpu().numpy()), depths[0].cpu().numpy()
    t0 = time.perf_counter()
    fr = R.refine_frame(cameras[0], G, d, f, p, R.Margins())
    sec = time.perf_counter() - t0
    differ = {key: int((got[f].cpu().numpy() != fr[key]).sum()) for key, got in (("k", kk), ("sum", sm), ("cnt", cnt))}
    differ["out"] = int((out[f].cpu().numpy().view(np.uint32) != fr["out"].view(np.uint32)).sum())
    return dict(step="numpy", frame=f, w=a.w, h=a.h, numpy_one_frame_s=sec, accepted=int(fr["accepted"].sum()), pixels_that_differ=differ)


def write_md(path, res):
    g, n = res["gpu"], res.get("numpy")
    best = g["call_ms_best"]
    lines = ["| quantity | value |", "|---|---|",
             f"| shape | {g['seqs']} sequences x {g['frames']} cameras x {g['w']} x {g['h']}, N = {g['ssd_win']}, K = {g['steps']}, window of {g['ref_frm_count']} frames |",
             f"| call, warm (HIP events, {len(g['call_ms'])} calls) | {', '.join(f'{m:.2f}' for m in g['call_ms'])} ms; best {best:.2f} ms |",
             f"| per frame | {best / (g['seqs'] * g['frames']):.3f} ms |",
             f"| pixels / with a winner / accepted | {g['pixels']} / {g['pixels_with_a_winner']} / {g['accepted']} |",
             f"| grey differences rule 5 asks for at most (no reuse between hypotheses) | {g['grey_differences_by_rule_5']:.3e}; {g['grey_differences_by_rule_5'] / best / 1e6:.1f} G/s at the best call |",
             f"| workgroups of the main launch | {g['tiles']} of 256 threads |",
             f"| two calls give the same bytes | {g['runs_identical']} |"]
    if n:
        lines += [f"| numpy restatement, ONE frame ({n['w']} x {n['h']}, CPU) | {n['numpy_one_frame_s']:.1f} s |",
                  f"| pixels of that frame that differ from the GPU (k / sum / cnt / out bits) | {n['pixels_that_differ']['k']} / {n['pixels_that_differ']['sum']} / "
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
               "--calls", str(a.calls)]
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
