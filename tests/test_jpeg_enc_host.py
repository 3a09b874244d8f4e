"""The JPEG encoder without a GPU: the restatement tests/ref_jpeg_enc.py (rules E1-E9 of include/mvs.h) against the streams Pillow wrote
(tests/golden/jpeg_enc), the goldens against a fresh Pillow encode where Pillow is importable, the round trip through the decoder's
restatement, csrc/jpeg_enc_rules.h run as a host program of its own (tests/jpeg_enc_rules.cpp) against the restatement — plain, and under
the address and undefined-behaviour sanitizers —, the depth preview's restatement at its edges, and the host entries through ctypes."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import make_jpeg_enc_golden as G, ref_jpeg as R, ref_jpeg_enc as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = G.load_all()
NAMES = sorted(FIX)
E_INVALID, E_NO_DEVICE = -1, -4
_ENCODED = {}


def encoded(name):
    """the restatement on fixture ``name``, computed once -> (stream, coefficients, counters)"""
    if name not in _ENCODED:
        f = FIX[name]
        _ENCODED[name] = E.encode_all(f["pixels"], f["mode"], f["quality"], f["restart"])
    return _ENCODED[name]


def test_the_fixture_set_is_complete_and_small():
    assert NAMES == sorted(G.cases()) and len(NAMES) == 6 * 4 * 2 + 6
    size = sum(os.path.getsize(os.path.join(G.HERE, f)) for f in os.listdir(G.HERE))
    assert size < 300 * 1024
    assert R.info(FIX["75x100_444_rst1"]["jpg"])["n_segments"] == 130
    assert R.info(FIX["33x50_420_rstrow"]["jpg"])["restart_interval"] == 4 and R.info(FIX["33x50_420_rst2"]["jpg"])["restart_interval"] == 2


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_equals_pillow(name):
    got, want = encoded(name)[0], FIX[name]["jpg"]
    print(name, len(got), "bytes, Pillow", len(want))
    assert got == want


def test_the_fixtures_cover_every_branch():
    """from the restatement's own counters: a stuffed FF, a ZRL, a dummy column and a dummy row, an interval that ended with padding and
    one that ended byte-aligned, and a 4:2:0 size with H mod 16 in 1 .. 8 (where the order of E3 decides the chroma bytes)"""
    total = {}
    for name in NAMES:
        for k, v in encoded(name)[2].items():
            total[k] = total.get(k, 0) + v
    print(total)
    for k in ("stuffed", "zrl", "dummy_col", "dummy_row", "padded_end", "aligned_end"):
        assert total[k] > 0, k
    assert any(FIX[n]["mode"] == "420" and 1 <= FIX[n]["pixels"].shape[0] % 16 <= 8 for n in NAMES)
    x = FIX["8x9_420_q95"]["pixels"]                                  # ... and there the other order does give other bytes
    hmax = vmax = 2
    cb = E.colour(x)[1]
    early = E.component_plane(E._extend(cb, 16, 16), 2, 2, hmax, vmax)
    assert not np.array_equal(early, E.component_plane(cb, 2, 2, hmax, vmax))


def test_the_goldens_are_what_pillow_encodes_today():
    pytest.importorskip("PIL")
    for name, (h, w, mode, q, r) in G.cases().items():
        a = G.pixels(h, w, mode)
        assert np.array_equal(a, FIX[name]["pixels"]), name
        data = G.pillow_encode(a, mode, q, r)
        assert data == FIX[name]["jpg"], name
        if FIX[name]["decoded"] is not None:
            assert np.array_equal(G.pillow_decode(data), FIX[name]["decoded"]), name


@pytest.mark.parametrize("name", [n for n in NAMES if FIX[n]["decoded"] is not None])
def test_the_round_trip_restatement(name):
    """ref_jpeg.decode(ref_jpeg_enc.encode(x)) is what Pillow decodes from Pillow's stream"""
    want = FIX[name]["decoded"]
    want = np.stack([want] * 3, axis=2) if want.ndim == 2 else want
    assert np.array_equal(R.decode(encoded(name)[0], "RGB"), want)


def test_channel_order_and_restart_row():
    f = FIX["33x50_420_q95"]
    assert E.encode(np.ascontiguousarray(f["pixels"][..., ::-1]), "420", 95, 0, "BGR") == f["jpg"]
    g = FIX["33x50_420_rstrow"]
    assert E.encode(g["pixels"], "420", 75, E.ROW) == g["jpg"]


# ------------------------------------------------------------------ the shared rules as a program ----
def _build(tmp_path, sanitize):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / ("jpeg_enc_rules_san" if sanitize else "jpeg_enc_rules"))
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "jpeg_enc_rules.cpp"), "-o", exe])
    return exe


def _cases():
    """-> [(what, pixels, mode, quality, restart, order)]: every fixture, then W or H of 1, 7, 8, 9, 15, 16, 17 in every mode"""
    out = [(n, FIX[n]["pixels"], FIX[n]["mode"], FIX[n]["quality"], FIX[n]["restart"], "RGB") for n in NAMES]
    rng = np.random.default_rng(28)
    edge = (1, 7, 8, 9, 15, 16, 17)
    for i, s in enumerate(edge):
        for k, mode in enumerate(G.MODES):
            for h, w in ((s, edge[(i + k + 1) % 7]), (edge[(i + 2 * k + 3) % 7], s)):
                a = rng.integers(0, 256, (h, w) if mode == "grey" else (h, w, 3), dtype=np.uint8)
                out.append((f"{h}x{w}_{mode}", a, mode, (35, 90)[(i + k) % 2], (0, 1, E.ROW)[(i + k) % 3], ("RGB", "BGR")[i % 2]))
    return out


def _run(exe, tmp_path, cases):
    return run_records(exe, tmp_path, [((a.shape[1], a.shape[0], 1 if mode == "grey" else 3, int(order == "RGB"), q, 420 if mode == "grey" else int(mode), r),
                                        np.ascontiguousarray(a).tobytes()) for _, a, mode, q, r, order in cases])


def run_records(exe, tmp_path, cases):
    """cases: [((w, h, chan, rgb, quality, sampling, restart_interval), the bytes behind them)], the records of the program's pack format
    (chan -1 or -3: a coefficient record, tests/test_jpeg_coef_host.py) -> [(stream, coefficients)]"""
    pack, out = str(tmp_path / "pack.bin"), str(tmp_path / "out.bin")
    with open(pack, "wb") as fh:
        fh.write(struct.pack("<q", len(cases)))
        for head, body in cases:
            fh.write(struct.pack("<7i", *head))
            fh.write(body)
    run = subprocess.run([exe, pack, out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and f"jpeg enc rules ok {len(cases)}" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    raw, p, res = open(out, "rb").read(), 0, []
    for _ in cases:
        (n,) = struct.unpack_from("<q", raw, p)
        data = raw[p + 8:p + 8 + n]
        p += 8 + n
        (nc,) = struct.unpack_from("<q", raw, p)
        res.append((data, np.frombuffer(raw, np.int16, nc, p + 8)))
        p += 8 + 2 * nc
    assert p == len(raw)
    return res


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_shared_rules_equal_the_restatement(tmp_path, sanitize):
    """the program, not a library loaded into Python: streams and coefficient blocks of every fixture and of the edge sizes are exactly
    the restatement's, and the sanitized build ends without a report"""
    cases = _cases()
    res = _run(_build(tmp_path, sanitize), tmp_path, cases)
    for (what, a, mode, q, r, order), (data, coef) in zip(cases, res):
        want, wc, _ = encoded(what) if what in FIX else E.encode_all(a, mode, q, r, order)
        assert np.array_equal(coef, np.concatenate([c.reshape(-1) for c in wc])), what
        assert data == want, what
        if what in FIX:
            assert data == FIX[what]["jpg"], what


# ------------------------------------------------------------------ depth preview ----
def test_the_depth_preview_restatement_at_its_edges():
    d = np.array([[0.5, 1.0, -1.0, np.nan], [2.5, 0.0, np.inf, -0.0]], np.float32)
    assert E.depth_preview(d).tolist() == [[51, 102, 255, 255], [255, 0, 255, 0]]
    assert E.depth_preview(np.full((2, 3), 0.25, np.float32)).tolist() == [[0] * 3] * 2       # d_max == d_min
    assert E.depth_preview(np.array([[-1.0, np.nan]], np.float32)).tolist() == [[255, 255]]    # no valid pixel
    rng = np.random.default_rng(3)
    d = rng.random((5, 7)).astype(np.float32)
    p = E.depth_preview(d)
    assert p.max() == 255 and p.min() == 0 and (p == 255).sum() == 1                           # only d_max reaches 255


# ------------------------------------------------------------------ the host entries ----
def test_the_entries_without_a_device():
    from multiviewstitch_amd import _lib as L, processor as P
    lib = L.lib()
    for name in ("mvs_jpeg_encode", "mvs_jpeg_encode_dev", "mvs_jpeg_encode_bound", "mvs_jpeg_encode_default_params", "mvs_jpeg_roundtrip",
                 "mvs_jpeg_roundtrip_dev", "mvs_depth_preview", "mvs_depth_preview_dev", "mvs_processor_save_views", "mvs_processor_depth_previews",
                 "mvs_test_jpeg_encode_timed"):
        assert hasattr(lib, name) and name in L.EXPORTS
    prm = P.jpeg_encode_params()
    assert (prm.quality, prm.sampling, prm.restart_interval) == (95, 420, 0)
    for name in NAMES:                                               # the bound holds for every golden stream
        f = FIX[name]
        h, w = f["pixels"].shape[:2]
        order = "GREY" if f["mode"] == "grey" else "RGB"
        bound = P.JpegEncodeBound(w, h, f["quality"], "420" if f["mode"] == "grey" else f["mode"], f["restart"], order)
        assert bound >= len(f["jpg"]), name
    x = np.zeros((2, 8, 9, 3), np.uint8)
    bad = [dict(quality=0), dict(quality=101), dict(sampling=411), dict(restart_interval=-1), dict(restart_interval=65536 + 1)]
    for kw in bad:                                                   # E1, reported before a device is needed
        args = dict(quality=95, sampling=420, restart_interval=0)
        args.update(kw)
        p = P.jpeg_encode_params(**args)
        off = np.zeros(3, np.int64)
        out = np.zeros(64, np.uint8)
        assert lib.mvs_jpeg_encode(2, 9, 8, L.ptr(x), 0, C.byref(p), L.ptr(off), L.ptr(out), 64) == E_INVALID, kw
        assert lib.mvs_jpeg_roundtrip(2, 9, 8, L.ptr(x), 0, C.byref(p), L.ptr(np.zeros_like(x))) == E_INVALID, kw
        assert lib.mvs_jpeg_encode_bound(9, 8, 0, C.byref(p)) == E_INVALID, kw
    p = P.jpeg_encode_params()
    off, out = np.zeros(3, np.int64), np.zeros(64, np.uint8)
    for n, w, h, flags in ((0, 9, 8, 0), (65536, 9, 8, 0), (2, 0, 8, 0), (2, 9, 65536, 0), (2, 9, 8, 4)):
        assert lib.mvs_jpeg_encode(n, w, h, L.ptr(x), flags, C.byref(p), L.ptr(off), L.ptr(out), 64) == E_INVALID, (n, w, h, flags)
    assert lib.mvs_jpeg_encode(2, 9, 8, None, 0, C.byref(p), L.ptr(off), L.ptr(out), 64) == E_INVALID
    assert lib.mvs_depth_preview(0, 9, 8, L.ptr(np.zeros(72, np.float32)), L.ptr(out)) == E_INVALID
    assert lib.mvs_processor_depth_previews(b"/nowhere", b"Other", 1, 9, 8, None) == E_INVALID
    with pytest.raises(L.MvsError) as e:
        P.EncodeJpegs(x, sampling="411")
    assert e.value.code == E_INVALID
    if L.device_count() == 0:
        for call in (lambda: P.EncodeJpegs(x), lambda: P.JpegRoundTrip(x), lambda: P.DepthPreview(np.zeros((1, 8, 9), np.float32))):
            with pytest.raises(L.MvsError) as e:
                call()
            assert e.value.code == E_NO_DEVICE
