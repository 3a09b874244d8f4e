"""First timing of the overlay pictures on the GPU (csrc/overlay.hip) at scan scale: the match pictures of one sequence pair, 16 x 16 frame
pairs of 640 x 480 with 200 matches each (256 canvases of 640 x 960), and the SIFT pictures of 128 views with 1 500 keys each, warm.

The script is a driver: the step that uses the GPU is a child process under its own time limit.
  gpu   match: through mvs_test_match_overlays_timed the host list build and the draw launch alone (HIP events); the whole
        mvs_match_overlays_dev call (host clock around the entry, which returns with the work complete); draw + mvs_jpeg_encode_dev; the
        file form mvs_processor_match_overlays into a scratch directory; a hipMemcpyAsync of the draw launch's bytes (one read and one
        write per pixel) in the same run; the numpy restatement (tests/ref_overlay.py) for one canvas; two draws compared byte for byte
        and one canvas against the restatement.  sift: the whole mvs_sift_overlays_dev call, in place, and the file form.
It prints one JSON line and, with --md, writes the tables of profiles/r30/overlay.md.  No time is a pass criterion."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_jpeg import frame, timed  # noqa: E402

LIMIT = 540                                                               # seconds for the GPU step
COPY_CEILING_TBS = 4.77                                                   # profiles/r16/poisson.md: the 1 GiB device-to-device copy


def inputs(a):
    rng = np.random.default_rng(30)
    imgs1 = np.stack([frame(i, a.w, a.h) for i in range(a.frames)])
    imgs2 = np.stack([frame(16 + i, a.w, a.h) for i in range(a.frames)])
    matches = [[np.stack([rng.integers(0, a.w, a.matches), rng.integers(0, a.h, a.matches), rng.integers(0, a.w, a.matches),
                          rng.integers(0, a.h, a.matches)], axis=1).astype(np.int32) for _ in range(a.frames)] for _ in range(a.frames)]
    views = np.stack([frame(32 + i % 16, a.w, a.h) for i in range(a.views)])
    keys = [(rng.random((a.keys, 4)) * [a.w, a.h, 4, 6]).astype(np.float32) for _ in range(a.views)]
    return imgs1, imgs2, matches, views, keys


def step_gpu(a):
    import ctypes as C
    import torch
    from multiviewstitch_amd import _lib as L, processor as P
    from tests import ref_overlay as R
    lib = L.lib()
    imgs1, imgs2, matches, views, keys = inputs(a)
    n = a.frames * a.frames
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(m) for row in matches for m in row])
    flat = np.ascontiguousarray(np.concatenate([m for row in matches for m in row]))
    d1, d2 = torch.as_tensor(imgs1).to("cuda"), torch.as_tensor(imgs2).to("cuda")
    out = torch.empty((n, 2 * a.h, a.w, 3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = L.ptr(st.cuda_stream)
    margs = (a.frames, a.frames, a.w, a.h, L.ptr(d1), L.ptr(d2), L.ptr(off), L.ptr(flat), None, L.ptr(out))

    def draw():
        L.check(lib.mvs_match_overlays_dev(*margs, s))
    draw()                                                                # warm-up
    first = out.clone()
    whole = timed(draw, a.calls)
    same = bool(torch.equal(first, out))
    parts = []
    for _ in range(a.calls):
        ms = (C.c_double * 2)()
        L.check(lib.mvs_test_match_overlays_timed(*margs, s, ms))
        parts.append(list(ms))
    t0 = time.perf_counter()
    ref = R.draw(np.concatenate([imgs1[0], imgs2[1]], axis=0), R.match_prims(matches[0][1], a.h, _rng_after(R, len(matches[0][0]))))
    numpy_ms = (time.perf_counter() - t0) * 1e3
    canvas_ok = bool(np.array_equal(out[1].cpu().numpy(), ref))
    zoff, empty = np.zeros(n + 1, np.int64), []                          # empty lists: the pixel path alone, the stack as a copy
    for _ in range(a.calls):
        ms = (C.c_double * 2)()
        L.check(lib.mvs_test_match_overlays_timed(*margs[:6], L.ptr(zoff), L.ptr(flat), None, L.ptr(out), s, ms))
        empty.append(ms[1])
    plain_ok = bool(np.array_equal(out[1].cpu().numpy(), np.concatenate([imgs1[0], imgs2[1]], axis=0)))
    nbytes = out.numel()
    other = torch.empty_like(out)
    copy_ms = []
    for _ in range(a.calls + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record()
            other.copy_(out, non_blocking=True)                           # hipMemcpyAsync device to device: reads and writes nbytes
            e1.record()
        st.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    del other
    prm = P.jpeg_encode_params()
    joff = np.zeros(n + 1, np.int64)
    cap = 512 << 20
    data = torch.empty(cap, dtype=torch.uint8, device="cuda")

    def draw_encode():
        draw()
        L.check(lib.mvs_jpeg_encode_dev(n, a.w, 2 * a.h, L.ptr(out), L.JPEG_BGR, C.byref(prm), L.ptr(joff), L.ptr(data), cap, s))
    draw_encode()
    both = timed(draw_encode, a.calls)
    stream_bytes = int(joff[n])
    with tempfile.TemporaryDirectory() as tmp:
        def files():
            P.MatchOverlayFiles(os.path.join(tmp, "Match"), 0, imgs1, imgs2, matches)
        files()
        file_ms = timed(files, max(2, a.calls // 2))
        blob = data[:stream_bytes].cpu().numpy()
        files_ok = all(open(os.path.join(tmp, "Match", f"match0_{c // a.frames}_{c % a.frames}.jpg"), "rb").read() == blob[joff[c]:joff[c + 1]].tobytes()
                       for c in range(0, n, 37))
    match = dict(canvases=n, matches_per_pair=a.matches, pixel_bytes=nbytes, call_ms=whole, parts_ms=parts, runs_identical=same,
                 canvas_equals_restatement=canvas_ok, empty_draw_ms=empty, empty_is_the_stack=plain_ok,
                 numpy_one_canvas_ms=numpy_ms, memcpy_ms=copy_ms[1:], draw_encode_ms=both,
                 stream_bytes=stream_bytes, file_form_ms=file_ms, files_equal_draw_encode=files_ok)
    del out, data, first
    # ---- SIFT form
    koff = np.zeros(a.views + 1, np.int64)
    koff[1:] = np.cumsum([len(k) for k in keys])
    kflat = np.ascontiguousarray(np.concatenate(keys))
    dv = torch.as_tensor(views).to("cuda")
    sout = torch.empty_like(dv)

    def sift():
        L.check(lib.mvs_sift_overlays_dev(a.views, a.w, a.h, L.ptr(dv), L.ptr(koff), L.ptr(kflat), L.ptr(sout), s))
    sift()
    sift_ms = timed(sift, a.calls)
    sift_ok = bool(np.array_equal(sout[3].cpu().numpy(), R.sift_canvases(views[3:4], keys[3:4])[0]))
    with tempfile.TemporaryDirectory() as tmp:
        v5 = views.reshape((a.views // 4, 4) + views.shape[1:])

        def sfiles():
            P.SiftOverlayFiles(tmp, "Sift", v5, keys)
        sfiles()
        sfile_ms = timed(sfiles, max(2, a.calls // 2))
    sift_r = dict(views=a.views, keys_per_view=a.keys, pixel_bytes=int(dv.numel()), call_ms=sift_ms, view_equals_restatement=sift_ok, file_form_ms=sfile_ms)
    return dict(step="gpu", w=a.w, h=a.h, frames=a.frames, calls=a.calls, device=torch.cuda.get_device_name(0), match=match, sift=sift_r)


def _rng_after(R, matches_before):
    """the generator as pair (0, 1) finds it: 6 draws per match of pair (0, 0)"""
    g = R.Rng()
    for _ in range(6 * matches_before):
        g.next()
    return g


def write_md(path, res):
    g = res["gpu"]
    m, sf = g["match"], g["sift"]
    med = lambda v: float(np.median(v))                                 # noqa: E731
    row = lambda name, v, per: f"| {name} | {med(v):.2f} ({min(v):.2f} - {max(v):.2f}) | {med(v) / per:.4f} |"   # noqa: E731
    p = np.asarray(m["parts_ms"])
    draw_ms, copy_ms = med(p[:, 1]), med(m["memcpy_ms"])
    moved = 2 * m["pixel_bytes"]
    tiles = -(-g["w"] // 16) * -(-2 * g["h"] // 16)
    listb = tiles * m["canvases"] * 3 * m["matches_per_pair"] * 24
    lines = [f"Device: {g['device']}.  Shape: {g['frames']} x {g['frames']} frame pairs of {g['w']} x {g['h']} with {m['matches_per_pair']} matches each: "
             f"{m['canvases']} canvases of {g['w']} x {2 * g['h']}, {m['pixel_bytes'] / 1e6:.0f} MB of pixels; {g['calls']} timed calls after one warm-up call, "
             "medians (min - max); host clock around the entry, which returns with the work complete, except the draw launch and the copy (device events).", "",
             "### match pictures", "", "| quantity | per call, ms | per canvas, ms |", "|---|---|---|",
             row("list build on the host (O6 and the three primitives per match)", p[:, 0], m["canvases"]),
             row("draw launch alone (k_ovl_draw, HIP events)", p[:, 1], m["canvases"]),
             row("draw launch with empty lists (the pixel path alone: the stack as a copy)", m["empty_draw_ms"], m["canvases"]),
             row("mvs_match_overlays_dev, whole call (build, upload of the lists, launch)", m["call_ms"], m["canvases"]),
             row("hipMemcpyAsync device to device of the same pixel bytes, same run", m["memcpy_ms"], m["canvases"]),
             row("draw + mvs_jpeg_encode_dev", m["draw_encode_ms"], m["canvases"]),
             row("mvs_processor_match_overlays (upload, draw, encode, download of the streams, 256 files)", m["file_form_ms"], m["canvases"]),
             f"| numpy restatement, ONE canvas (tests/ref_overlay.py, one host thread) | {m['numpy_one_canvas_ms']:.1f} | {m['numpy_one_canvas_ms']:.1f} |", "",
             f"The draw launch reads every pixel once and writes it once: {moved / 1e9:.3f} GB in {draw_ms:.3f} ms = {moved / draw_ms / 1e9:.2f} TB/s, "
             f"{100 * moved / draw_ms / 1e9 / COPY_CEILING_TBS:.0f} % of the {COPY_CEILING_TBS} TB/s copy ceiling of profiles/r16/poisson.md; the copy of the same bytes in "
             f"this run took {copy_ms:.3f} ms = {moved / copy_ms / 1e9:.2f} TB/s, so the draw is {draw_ms / copy_ms:.2f} x the copy.",
             f"What the launch reads beside the pixels, computed from the shapes (no counter run was made): every tile's workgroup reads its canvas's whole "
             f"list, {3 * m['matches_per_pair']} primitives of 24 bytes, so {tiles} tiles x {m['canvases']} canvases read {listb / 1e9:.2f} GB of lists through "
             f"the caches, {listb / moved:.1f} x the pixel bytes, and test {tiles * m['canvases'] * 3 * m['matches_per_pair'] / 1e9:.2f} G primitive-tile pairs.",
             f"Streams: {m['stream_bytes'] / 1e6:.1f} MB.  Two draws give the same bytes: {m['runs_identical']}.  Canvas (0, 1) equals the restatement: "
             f"{m['canvas_equals_restatement']}.  Every 37th file equals its stream of draw + encode: {m['files_equal_draw_encode']}.", "",
             "### SIFT pictures", "", f"{sf['views']} views of {g['w']} x {g['h']} with {sf['keys_per_view']} keys each, {sf['pixel_bytes'] / 1e6:.0f} MB of pixels.", "",
             "| quantity | per call, ms | per view, ms |", "|---|---|---|",
             row("mvs_sift_overlays_dev, whole call (rounding and list build on the host, upload, launch)", sf["call_ms"], sf["views"]),
             row("mvs_processor_sift_overlays (upload, draw in place, encode, download of the streams, files)", sf["file_form_ms"], sf["views"]), "",
             f"View 3 equals the restatement: {sf['view_equals_restatement']}.", ""]
    with open(path, "w") as fh:
        fh.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--matches", type=int, default=200)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--keys", type=int, default=1500)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--step", choices=("gpu",), help="run the step in this process (the driver starts it)")
    ap.add_argument("--md", help="write the tables to this file")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step_gpu(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu"] + [x for k in ("frames", "w", "h", "matches", "views", "keys", "calls")
                                                                           for x in (f"--{k}", str(getattr(a, k)))]
    try:
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(failed="gpu", why=f"no result within {LIMIT} s")))
        return 1
    if run.returncode != 0:
        print(json.dumps(dict(failed="gpu", rc=run.returncode, stderr=run.stderr[-2000:])))
        return 1
    res = dict(gpu=json.loads(run.stdout.strip().splitlines()[-1]))
    if a.md:
        write_md(a.md, res)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
