"""First timing of the JPEG encoder on the GPU (csrc/jpeg_enc.hip) at scan scale: 8 sequences x 16 frames of 640 x 480, 4:2:0, quality 95,
pixels in HBM, once without restart markers and once with one MCU row per interval, through mvs_jpeg_encode_dev, warm.  Beside it the
round-trip entry (mvs_jpeg_roundtrip_dev) and what it replaces, encode + decode.

The script is a driver: the step that uses the GPU is a child process under its own time limit.
  gpu     per call: the whole mvs_jpeg_encode_dev call (host clock around the entry, which returns with the work complete), and through
          mvs_test_jpeg_encode_timed its parts: plan + header (host) and the three launch sets by HIP events; two calls are compared
          byte for byte, and where Pillow is importable every 7th stream with Pillow's
  pillow  what a caller does today, where Pillow is importable: the download of the pixels, then Pillow encoding them on 1 and on 16 host
          threads; otherwise the result says that it was not
It prints one JSON line and, with --md, writes the tables of profiles/r28/jpeg_encode.md.  No time is a pass criterion."""
import argparse
import io
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_jpeg import frame, have_pillow, timed  # noqa: E402

LIMIT = 420                                                               # seconds for the GPU step
FORMS = ("plain", "rstrow")


def step_gpu(a):
    import ctypes as C
    import torch
    from multiviewstitch_amd import _lib as L, processor as P
    lib = L.lib()
    n = a.seqs * a.frames
    host = np.stack([frame(i % 16, a.w, a.h) for i in range(n)])         # 16 distinct frames, taken in turn; R G B
    px = torch.as_tensor(host).to("cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    res = dict(step="gpu", seqs=a.seqs, frames=a.frames, w=a.w, h=a.h, calls=a.calls, pillow=have_pillow(), forms={})
    for form in FORMS:
        prm = P.jpeg_encode_params(quality=95, sampling=420, restart_interval=L.JPEG_RESTART_ROW if form == "rstrow" else 0)
        off = np.zeros(n + 1, np.int64)
        cap = n * int(lib.mvs_jpeg_encode_bound(a.w, a.h, L.JPEG_RGB, C.byref(prm)))
        data = torch.empty(cap, dtype=torch.uint8, device="cuda")

        def call():
            L.check(lib.mvs_jpeg_encode_dev(n, a.w, a.h, L.ptr(px), L.JPEG_RGB, C.byref(prm), L.ptr(off), L.ptr(data), cap, L.ptr(st.cuda_stream)))
        call()                                                            # warm-up
        total = int(off[n])
        first, first_off = data[:total].clone(), off.copy()
        whole = timed(call, a.calls)
        same = bool(torch.equal(first, data[:total])) and bool(np.array_equal(first_off, off))
        parts = []
        for _ in range(a.calls):
            ms = (C.c_double * 4)()
            L.check(lib.mvs_test_jpeg_encode_timed(n, a.w, a.h, L.ptr(px), L.JPEG_RGB, C.byref(prm), L.ptr(off), L.ptr(data), cap, L.ptr(st.cuda_stream), ms))
            parts.append(list(ms))
        out = torch.empty((n, a.h, a.w, 3), dtype=torch.uint8, device="cuda")

        def roundtrip():
            L.check(lib.mvs_jpeg_roundtrip_dev(n, a.w, a.h, L.ptr(px), L.JPEG_RGB, C.byref(prm), L.ptr(out), L.ptr(st.cuda_stream)))
        roundtrip()
        rt = timed(roundtrip, a.calls)
        blob = first.cpu().numpy()

        def decode():
            L.check(lib.mvs_jpeg_decode_dev(n, L.ptr(first_off), L.ptr(blob), L.JPEG_RGB, L.ptr(dec), L.ptr(st.cuda_stream)))
        dec = torch.empty_like(out)
        decode()
        r = dict(bytes=total, intervals=P.JpegInfo(blob[:first_off[1]].tobytes())["n_segments"] * n, call_ms=whole, parts_ms=parts, runs_identical=same,
                 roundtrip_ms=rt, decode_ms=timed(decode, a.calls), roundtrip_equals_decode_of_encode=bool(torch.equal(out, dec)))
        if have_pillow():
            from PIL import Image
            kw = dict(restart_marker_rows=1) if form == "rstrow" else {}

            def enc(x):
                b = io.BytesIO()
                Image.fromarray(x).save(b, "JPEG", quality=95, subsampling=2, **kw)
                return b.getvalue()
            r["streams_that_differ_from_pillow"] = int(sum(enc(host[i]) != blob[first_off[i]:first_off[i + 1]].tobytes() for i in range(0, n, 7)))
            r["pillow_1_thread_ms"] = timed(lambda: [enc(x) for x in host], a.calls)
            with ThreadPoolExecutor(16) as ex:
                r["pillow_16_threads_ms"] = timed(lambda: list(ex.map(enc, host)), a.calls)
            back = np.empty_like(host)

            def download():
                torch.from_numpy(back).copy_(px)
                torch.cuda.synchronize()
            download()
            r["pixel_download_ms"] = timed(download, a.calls)
        res["forms"][form] = r
    return res


def write_md(path, res):
    g = res["gpu"]
    n = g["seqs"] * g["frames"]
    med = lambda v: float(np.median(v))                                 # noqa: E731
    lines = [f"Shape: {g['seqs']} x {g['frames']} frames of {g['w']} x {g['h']}, 4:2:0, quality 95, pixels in HBM; {g['calls']} timed calls after one warm-up "
             "call, medians (min - max); host clock around the entry except the three launch sets (HIP events).", ""]
    if not g["pillow"]:
        lines += ["Pillow was not importable where this ran: no host encoder was timed and no stream was compared with Pillow's here.", ""]
    for form, r in g["forms"].items():
        p = np.asarray(r["parts_ms"])
        lines += [f"### {form}: {r['bytes'] / 1e6:.2f} MB of streams, {r['intervals']} intervals", "", "| quantity | per call, ms | per frame, ms |", "|---|---|---|"]
        rows = [("mvs_jpeg_encode_dev, whole call", r["call_ms"])]
        rows += [(name, p[:, i]) for i, name in enumerate(("host plan + header", "launch set 1: colour, downsample, FDCT, quantise",
                                                            "launch set 2: bit lengths, scans, bits (with the wait for the unstuffed size)",
                                                            "launch set 3: FF count, scan, offsets, stuffing, headers (with the wait for the offsets)"))]
        rows += [("mvs_jpeg_roundtrip_dev", r["roundtrip_ms"]), ("mvs_jpeg_decode_dev of the streams (encode + decode = this + the first row)", r["decode_ms"])]
        for key, name in (("pillow_1_thread_ms", "Pillow, 1 host thread"), ("pillow_16_threads_ms", "Pillow, 16 host threads"),
                          ("pixel_download_ms", f"download of the pixels ({n * g['w'] * g['h'] * 3 / 1e6:.0f} MB, pageable)")):
            if key in r:
                rows.append((name, r[key]))
        for name, v in rows:
            lines.append(f"| {name} | {med(v):.2f} ({min(v):.2f} - {max(v):.2f}) | {med(v) / n:.4f} |")
        lines += ["", f"Two calls give the same bytes: {r['runs_identical']}.  The round trip equals decode of encode: {r['roundtrip_equals_decode_of_encode']}." +
                  (f"  Streams that differ from Pillow's among every 7th frame: {r['streams_that_differ_from_pillow']}." if "streams_that_differ_from_pillow" in r else ""), ""]
    with open(path, "w") as fh:
        fh.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--step", choices=("gpu",), help="run the step in this process (the driver starts it)")
    ap.add_argument("--md", help="write the tables to this file")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step_gpu(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu", "--seqs", str(a.seqs), "--frames", str(a.frames), "--w", str(a.w), "--h", str(a.h),
           "--calls", str(a.calls)]
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
