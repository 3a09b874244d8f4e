"""First timing of the JPEG decoder on the GPU (csrc/jpeg.hip) at scan scale: 8 sequences x 16 frames of 640 x 480, 4:2:0, quality 90, once
without restart markers (one wave per image in the entropy launch) and once with restart_marker_rows=1 (one wave per MCU row), through
mvs_jpeg_decode_dev, warm.  The frames are encoded by Pillow where it is importable; otherwise they are read from --dir (sub-folders
`plain` and `rstrow` of *.jpg, e.g. written by `--write-dir` on a machine that has Pillow); with neither the script says so and exits 0.

The script is a driver: the step that uses the GPU is a child process under its own time limit.
  gpu     per call: the whole mvs_jpeg_decode_dev call (host clock around the entry, which returns with the work complete), and through
          mvs_test_jpeg_decode_timed its parts: the host header walk, allocation + upload, and the three launch sets by HIP events;
          the result of the first call is compared with Pillow's pixels where Pillow exists, and two calls byte for byte
  pillow  what a caller does today: Pillow decoding the same streams on 1 and on 16 host threads, plus the upload of the decoded pixels
It prints one JSON line and, with --md, writes the table of profiles/r27/jpeg.md.  No time is a pass criterion."""
import argparse
import glob
import io
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 420                                                               # seconds for the GPU step
FORMS = ("plain", "rstrow")


def frame(i, w, h):
    """a smooth scene with texture, noise and a saturated patch; differs from frame to frame"""
    rng = np.random.default_rng(4000 + i)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.stack([128 + 70 * np.sin(x / (23.0 + c) + 0.1 * i) * np.cos(y / (31.0 - c) + c) + 30 * np.sin((x + 2 * y) / (5.0 + c)) for c in range(3)], 2)
    a += rng.normal(0, 6, (h, w, 3))
    a[h // 3:h // 2, w // 3:w // 2] = (250, 5, 250)
    return np.clip(a, 0, 255).astype(np.uint8)


def have_pillow():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def streams(a):
    """-> {form: [bytes]} or None"""
    n = a.seqs * a.frames
    if have_pillow():
        from PIL import Image
        out = {f: [] for f in FORMS}
        for i in range(n):
            im = Image.fromarray(frame(i % 16, a.w, a.h))                 # 16 distinct frames, taken in turn
            for form in FORMS:
                b = io.BytesIO()
                im.save(b, "JPEG", quality=90, subsampling=2, **({"restart_marker_rows": 1} if form == "rstrow" else {}))
                out[form].append(b.getvalue())
        return out
    if a.dir:
        out = {}
        for form in FORMS:
            files = sorted(glob.glob(os.path.join(a.dir, form, "*.jpg")))
            if not files:
                return None
            data = [open(f, "rb").read() for f in files]
            out[form] = [data[i % len(data)] for i in range(n)]
        return out
    return None


def timed(fn, calls):
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def step_gpu(a):
    import ctypes as C
    import torch
    from multiviewstitch_amd import _lib as L, processor as P
    src = streams(a)
    if src is None:
        return dict(step="gpu", skipped="no Pillow and no --dir with frames")
    res = dict(step="gpu", seqs=a.seqs, frames=a.frames, w=a.w, h=a.h, calls=a.calls, pillow=have_pillow(), forms={})
    st = torch.cuda.Stream()
    for form in FORMS:
        datas = src[form]
        n = len(datas)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(d) for d in datas])
        blob = np.frombuffer(b"".join(datas), np.uint8)
        info = P.JpegInfo(datas[0])
        out = torch.empty((n, a.h, a.w, 3), dtype=torch.uint8, device="cuda")
        lib = L.lib()

        def call():
            L.check(lib.mvs_jpeg_decode_dev(n, L.ptr(off), L.ptr(blob), L.JPEG_RGB, L.ptr(out), L.ptr(st.cuda_stream)))
        call()                                                            # warm-up
        first = out.clone()
        whole = timed(call, a.calls)
        same = bool(torch.equal(first, out))
        parts = []
        for _ in range(a.calls):
            ms = (C.c_double * 5)()
            L.check(lib.mvs_test_jpeg_decode_timed(n, L.ptr(off), L.ptr(blob), L.JPEG_RGB, L.ptr(out), L.ptr(st.cuda_stream), ms))
            parts.append(list(ms))
        r = dict(bytes=int(off[-1]), segments=info["n_segments"] * n, call_ms=whole, parts_ms=parts, runs_identical=same)
        if have_pillow():
            from PIL import Image
            host = first.cpu().numpy()
            dec = lambda d: np.asarray(Image.open(io.BytesIO(d)))      # noqa: E731
            r["bytes_that_differ_from_pillow"] = int(sum((host[i] != dec(datas[i])).sum() for i in range(0, n, 7)))
            r["pillow_1_thread_ms"] = timed(lambda: [dec(d) for d in datas], a.calls)
            with ThreadPoolExecutor(16) as ex:
                r["pillow_16_threads_ms"] = timed(lambda: list(ex.map(dec, datas)), a.calls)
            px = torch.from_numpy(np.stack([dec(d) for d in datas]))

            def upload():
                out.copy_(px)
                torch.cuda.synchronize()
            upload()
            r["pixel_upload_ms"] = timed(upload, a.calls)
        res["forms"][form] = r
    return res


def write_md(path, res):
    g = res["gpu"]
    n = g["seqs"] * g["frames"]
    med = lambda v: float(np.median(v))                                 # noqa: E731
    lines = [f"Shape: {g['seqs']} x {g['frames']} frames of {g['w']} x {g['h']}, 4:2:0, quality 90; {g['calls']} timed calls after one warm-up call, "
             "medians (min - max); host clock around the entry except the three launch sets (HIP events).", ""]
    for form, r in g["forms"].items():
        p = np.asarray(r["parts_ms"])
        lines += [f"### {form}: {r['bytes'] / 1e6:.2f} MB of streams, {r['segments']} segments", "", "| quantity | per call, ms | per frame, ms |", "|---|---|---|"]
        rows = [("mvs_jpeg_decode_dev, whole call", r["call_ms"])]
        rows += [(name, p[:, i]) for i, name in enumerate(("host header walk", "allocation + upload of the streams and tables", "launch set 1: entropy",
                                                            "launch set 2: dequantise + IDCT", "launch set 3: upsample + colour + crop"))]
        for key, name in (("pillow_1_thread_ms", "Pillow, 1 host thread"), ("pillow_16_threads_ms", "Pillow, 16 host threads"),
                          ("pixel_upload_ms", f"upload of the decoded pixels ({n * g['w'] * g['h'] * 3 / 1e6:.0f} MB, pageable)")):
            if key in r:
                rows.append((name, r[key]))
        for name, v in rows:
            lines.append(f"| {name} | {med(v):.2f} ({min(v):.2f} - {max(v):.2f}) | {med(v) / n:.4f} |")
        lines += ["", f"Two calls give the same bytes: {r['runs_identical']}." +
                  (f"  Bytes that differ from Pillow on every 7th frame: {r['bytes_that_differ_from_pillow']}." if "bytes_that_differ_from_pillow" in r else ""), ""]
    with open(path, "w") as fh:
        fh.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--dir", help="frames to read where Pillow is missing: <dir>/plain/*.jpg and <dir>/rstrow/*.jpg")
    ap.add_argument("--write-dir", help="encode the 16 distinct frames with Pillow into this folder and stop")
    ap.add_argument("--step", choices=("gpu",), help="run the step in this process (the driver starts it)")
    ap.add_argument("--md", help="write the tables to this file")
    a = ap.parse_args()
    if a.write_dir:
        a.seqs, a.frames = 1, 16
        for form, datas in streams(a).items():
            os.makedirs(os.path.join(a.write_dir, form), exist_ok=True)
            for i, d in enumerate(datas):
                open(os.path.join(a.write_dir, form, f"{i:05d}.jpg"), "wb").write(d)
        return 0
    if a.step:
        print(json.dumps(step_gpu(a)))
        return 0
    if not have_pillow() and not a.dir:
        print(json.dumps(dict(skipped="Pillow is not importable and no --dir was given: nothing to decode")))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu", "--seqs", str(a.seqs), "--frames", str(a.frames), "--w", str(a.w), "--h", str(a.h),
           "--calls", str(a.calls)] + (["--dir", a.dir] if a.dir else [])
    try:
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(failed="gpu", why=f"no result within {LIMIT} s")))
        return 1
    if run.returncode != 0:
        print(json.dumps(dict(failed="gpu", rc=run.returncode, stderr=run.stderr[-2000:])))
        return 1
    res = dict(gpu=json.loads(run.stdout.strip().splitlines()[-1]))
    if a.md and "forms" in res["gpu"]:
        write_md(a.md, res)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
