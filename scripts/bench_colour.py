"""First timing of the vertex colouring on the GPU (csrc/colour.hip) at scan scale: 8 sequences x 16 cameras of 640 x 480 on a ring
around a unit sphere, each sequence in a frame of its own, images and rasters resident in HBM, default parameters, through
mvs_colour_vertices_dev, warm.  The rasters are mvs_render_depth_views_dev of the geodesic sphere of frequency 74 (V = 54 762, the size of
the template); the vertices are that mesh's, and about 2 M seeded points of the same sphere with their radial normals (the size of the
Poisson model).

The script is a driver: every step that uses the GPU is a child process under its own time limit, and a step that fails or runs out of
time ends the run.
  gpu    at both vertex counts the _dev call between HIP events on its stream (--calls of them after two warm-up calls), once per kernel
         mapping (MVS_COLOUR_MAPPING = 1: a thread per vertex; 16: a row of 16 lanes per vertex), the mappings taken in turn, their
         outputs compared byte for byte; MVS_COLOUR_BEST and the call without rasters with the call's own mapping; in the same run
         mvs_visibility_cull_dev (MVS_CULL_ALL_SEQ) on the same points and cameras — the same projection loop without the gathers —
         and a device copy of the image and raster bytes
  files  mvs_processor_colour_model end to end on files: the OBJ of the template-sized mesh, SRT.txt and 128 JPEG frames (a smooth
         texture, written by the library's encoder), the second of two calls on a host clock
It prints one JSON line and, with --md, writes the table of profiles/r32/colour.md.  No time is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"gpu": 400, "files": 300}                                       # seconds per step


def build(a):
    """cameras per sequence, the chain, the mesh of the rasters"""
    from multiviewstitch_amd import scene as S
    from tests import colour_scenes as SC
    verts, faces = S.geodesic_sphere(a.mesh_n)
    n_views = a.seqs * a.frames
    scales = 1.0 + 0.02 * np.arange(a.seqs)
    Rs = np.stack([SC.rodrigues((1, 2, 3), 0.1 * k) for k in range(a.seqs)])
    ts = np.stack([[0.05 * k, -0.03 * k, 0.02 * k] for k in range(a.seqs)]).astype(np.float64)
    cameras = []
    for k in range(a.seqs):
        seq = []
        for i in range(a.frames):
            ang = 2 * np.pi * (k * a.frames + i) / n_views
            c = SC.look_at((4 * np.sin(ang), 0.4, -4 * np.cos(ang)), (0, 0, 0), fx=1.09 * a.w)
            c = S.Camera(c.fx, c.fy, a.w / 2 - 0.5, a.h / 2 - 0.5, c.R, c.t, a.w, a.h)
            seq.append(SC.local_camera(c, scales[k], Rs[k], ts[k]))
        cameras.append(seq)
    return np.ascontiguousarray(verts, np.float64), np.ascontiguousarray(faces, np.int32), cameras, scales, Rs, ts


def texture(n, h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([np.stack([(127 + 100 * np.sin(0.02 * xs + 0.3 * v + ch) * np.cos(0.03 * ys + ch)) for ch in range(3)], axis=2)
                     for v in range(n)]).astype(np.uint8)


def _timed(st, calls, fn, warm=2):
    import torch
    for _ in range(warm):
        fn()
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
    from multiviewstitch_amd import _lib as L, processor as P
    verts, faces, cameras, scales, Rs, ts = build(a)
    n, s, R, t, coff, cams = L.seq_tables(scales, Rs, ts, cameras)
    N, lib, st = int(coff[-1]), L.lib(), torch.cuda.current_stream()
    gen = torch.Generator(device="cuda").manual_seed(5)
    imgs = torch.randint(0, 256, (N, a.h, a.w, 3), dtype=torch.uint8, device="cuda", generator=gen)
    dv, df = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    ras = torch.empty((N, a.h, a.w), dtype=torch.float32, device="cuda")
    L.check(lib.mvs_render_depth_views_dev(L.ptr(dv), len(verts), L.ptr(df), len(faces), n, L.ptr(s), L.ptr(R), L.ptr(t), L.ptr(coff), cams, 0.01, 2000.0,
                                           L.ptr(ras), L.ptr(st.cuda_stream)))
    big = torch.randn((a.big, 3), dtype=torch.float64, device="cuda", generator=gen)
    big = (big / big.norm(dim=1, keepdim=True)).contiguous()
    res = dict(step="gpu", seqs=a.seqs, frames=a.frames, w=a.w, h=a.h, image_and_raster_bytes=int(imgs.numel() + 4 * ras.numel()),
               covered_pixels=int((ras > 0).sum()), sizes=[])
    prm, best = P.colour_params(), P.colour_params(flags=L.COLOUR_BEST)
    for pts in (dv, big):
        V = int(pts.shape[0])
        col = {m: torch.empty((V, 3), dtype=torch.uint8, device="cuda") for m in ("1", "16", "own")}
        cnt = {m: torch.empty(V, dtype=torch.int32, device="cuda") for m in ("1", "16", "own")}

        def call(m, p=prm, depths=ras):
            L.check(lib.mvs_colour_vertices_dev(L.ptr(pts), L.ptr(pts), V, n, L.ptr(s), L.ptr(R), L.ptr(t), L.ptr(coff), cams, L.ptr(imgs),
                                                L.ptr(depths) if depths is not None else None, C.byref(p), L.ptr(col[m]), L.ptr(cnt[m]), L.ptr(st.cuda_stream)))

        ms = {"1": [], "16": []}
        for rnd in range(2):                                             # the mappings in turn, twice
            for m in ("1", "16"):
                os.environ["MVS_COLOUR_MAPPING"] = m
                ms[m] += _timed(st, a.calls, lambda: call(m))
        os.environ.pop("MVS_COLOUR_MAPPING")
        own = _timed(st, a.calls, lambda: call("own"))
        own_best = _timed(st, a.calls, lambda: call("own", best))
        own_bare = _timed(st, a.calls, lambda: call("own", prm, None))
        call("own")
        keep = torch.empty(V, dtype=torch.uint8, device="cuda")
        seg, nk = np.asarray([0, V], np.int64), np.zeros(1, np.int64)
        cull = _timed(st, a.calls, lambda: L.check(lib.mvs_visibility_cull_dev(L.ptr(pts), L.ptr(seg), 1, n, L.ptr(s), L.ptr(R), L.ptr(t), L.ptr(coff), cams,
                                                                                L.CULL_ALL_SEQ, L.ptr(keep), L.ptr(nk), L.ptr(st.cuda_stream))))
        res["sizes"].append(dict(V=V, thread_per_vertex_ms=ms["1"], row_per_vertex_ms=ms["16"], own_choice_ms=own, best_flag_ms=own_best, no_rasters_ms=own_bare,
                                 visibility_cull_ms=cull, mappings_identical=bool(torch.equal(col["1"], col["16"]) and torch.equal(cnt["1"], cnt["16"])),
                                 own_identical=bool(torch.equal(col["own"], col["1"])), coloured=int((cnt["own"] > 0).sum()),
                                 accepted_pairs=int(cnt["own"].sum()), pairs=V * N))
    src = torch.empty(res["image_and_raster_bytes"], dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res["device_copy_ms"] = _timed(st, a.calls, lambda: dst.copy_(src))
    return res


def step_files(a):
    from multiviewstitch_amd import io as IO, processor as P
    verts, faces, cameras, scales, Rs, ts = build(a)
    with tempfile.TemporaryDirectory() as tmp:
        model, srt, out = (os.path.join(tmp, f) for f in ("deform.obj", "SRT.txt", "coloured.obj"))
        IO.WriteObj(model, verts, verts, faces)
        IO.write_srt_txt(srt, scales, Rs, ts)
        dirs = []
        for k in range(a.seqs):
            d = os.path.join(tmp, f"seq{k}") + os.sep
            os.mkdir(d)
            dirs.append(d)
            streams = P.EncodeJpegs(texture(a.frames, a.h, a.w), order="RGB")
            for i, blob in enumerate(streams):
                with open(os.path.join(d, f"{i:05d}.jpg"), "wb") as fh:
                    fh.write(bytes(blob))
        sec, n = [], 0
        for _ in range(2):
            t0 = time.perf_counter()
            n = P.ColourModelFiles(model, srt, dirs, cameras, out)
            sec.append(time.perf_counter() - t0)
        return dict(step="files", V=len(verts), F=len(faces), views=a.seqs * a.frames, call_s=sec, coloured=n, out_bytes=os.path.getsize(out))


def write_md(path, res):
    g, f = res["gpu"], res.get("files")
    lo = lambda v: f"{', '.join(f'{m:.3f}' for m in v)} ms; best {min(v):.3f} ms"
    lines = ["| quantity | value |", "|---|---|",
             f"| shape | {g['seqs']} sequences x {g['frames']} cameras x {g['w']} x {g['h']}, a chain per sequence, default parameters; "
             f"{g['image_and_raster_bytes']} bytes of images and rasters, {g['covered_pixels']} covered pixels |"]
    for z in g["sizes"]:
        lines += [f"| V = {z['V']}: a thread per vertex (HIP events, two rounds in turn) | {lo(z['thread_per_vertex_ms'])} |",
                  f"| V = {z['V']}: a row of 16 lanes per vertex | {lo(z['row_per_vertex_ms'])} |",
                  f"| V = {z['V']}: the call's own choice / with MVS_COLOUR_BEST / without rasters | best {min(z['own_choice_ms']):.3f} / "
                  f"{min(z['best_flag_ms']):.3f} / {min(z['no_rasters_ms']):.3f} ms |",
                  f"| V = {z['V']}: mvs_visibility_cull_dev, MVS_CULL_ALL_SEQ, same points and cameras, same run | {lo(z['visibility_cull_ms'])} |",
                  f"| V = {z['V']}: pairs / accepted pairs / coloured vertices | {z['pairs']} / {z['accepted_pairs']} / {z['coloured']} |",
                  f"| V = {z['V']}: both mappings give the same bytes / the call's own choice too | {z['mappings_identical']} / {z['own_identical']} |"]
    lines += [f"| device copy of the image and raster bytes | {lo(g['device_copy_ms'])} |"]
    if f:
        lines += [f"| mvs_processor_colour_model end to end (V = {f['V']}, F = {f['F']}, {f['views']} JPEG frames; host clock, first and second call) | "
                  f"{f['call_s'][0]:.2f} s, {f['call_s'][1]:.2f} s; {f['coloured']} vertices coloured, {f['out_bytes']} bytes written |"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--mesh-n", type=int, default=74, help="frequency of the geodesic sphere: V = 10 n^2 + 2")
    ap.add_argument("--big", type=int, default=2000000, help="points of the large case")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--step", choices=("gpu", "files"), help="run one step in this process (the driver starts these)")
    ap.add_argument("--skip-files", action="store_true")
    ap.add_argument("--md", help="write the table to this file")
    a = ap.parse_args()
    if a.step:
        print(json.dumps((step_gpu if a.step == "gpu" else step_files)(a)))
        return 0
    res = {}
    for step in ("gpu",) + (() if a.skip_files else ("files",)):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--seqs", str(a.seqs), "--frames", str(a.frames), "--w", str(a.w), "--h", str(a.h),
               "--mesh-n", str(a.mesh_n), "--big", str(a.big), "--calls", str(a.calls)]
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
