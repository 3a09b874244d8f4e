"""The JPEG decoder without a GPU: the restatement tests/ref_jpeg.py (rules J1-J7 of include/mvs.h) against the pixels Pillow decoded
(tests/golden/jpeg), the goldens against a fresh Pillow decode where Pillow is importable, csrc/jpeg_rules.h run as a host program of its
own (tests/jpeg_rules.cpp) against the restatement — plain, and under the address and undefined-behaviour sanitizers on truncated and
corrupted streams —, and the host entries through ctypes."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import make_jpeg_golden as G, ref_jpeg as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = G.load_all()
ACCEPTED = sorted(k for k, (_, px) in FIX.items() if px is not None)
REJECTED = {"17x23_progressive": "progressive", "17x23_cmyk": "components"}
E_IO, E_NO_DEVICE = -10, -4


def cut_scan(data):
    """the stream with the second half of its scan cut off and EOI appended (the scan-error case of the GPU tests)"""
    h = R.parse(data)
    first, end = h["segments"][0][0], h["segments"][-1][1]
    return data[:first + (end - first) // 2] + b"\xff\xd9"


def test_the_fixture_set_is_complete_and_small():
    assert len(ACCEPTED) == 5 * 4 * 2 + 8 and sorted(k for k in FIX if k not in ACCEPTED) == sorted(REJECTED)
    size = sum(os.path.getsize(os.path.join(G.HERE, f)) for f in os.listdir(G.HERE))
    assert size < 300 * 1024
    assert R.info(FIX["75x100_420_rst1"][0])["n_segments"] == 35 and R.info(FIX["75x100_444_rst1"][0])["n_segments"] == 130
    assert R.info(FIX["33x50_420_sof1"][0])["sof"] == 1 and R.info(FIX["33x50_420_rstrow"][0])["restart_interval"] == 4
    clamp = [int((FIX[k][1] == 255).sum() + (FIX[k][1] == 0).sum()) for k in ACCEPTED if not k.startswith(("1x1", "8x9"))]
    assert min(clamp) > 0                                            # every image from 17 x 23 on saturates somewhere


@pytest.mark.parametrize("name", ACCEPTED)
def test_the_restatement_equals_pillow(name):
    data, px = FIX[name]
    got = R.decode(data, "RGB")
    print(name, len(data), "bytes,", int((got != px).sum()), "differing bytes")
    assert got.shape == px.shape and np.array_equal(got, px)
    assert np.array_equal(R.decode(data, "BGR"), px[..., ::-1])


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_the_restatement_rejects(name):
    with pytest.raises(R.JpegError, match=REJECTED[name]):
        R.decode(FIX[name][0])


def test_the_goldens_are_what_pillow_decodes_today():
    pytest.importorskip("PIL")
    fresh = G.fixtures()
    assert sorted(fresh) == sorted(FIX)
    for name, (data, ok) in fresh.items():
        assert data == FIX[name][0], name                           # the encoder is as deterministic as the decoder
        if ok:
            px = G.pillow_pixels(data)
            px = np.stack([px] * 3, axis=2) if px.ndim == 2 else px
            assert np.array_equal(px, FIX[name][1]), name


# ------------------------------------------------------------------ the shared rules as a program ----
def _build(tmp_path, sanitize):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / ("jpeg_rules_san" if sanitize else "jpeg_rules"))
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "jpeg_rules.cpp"), "-o", exe])
    return exe


def _run(exe, tmp_path, streams):
    """-> per stream (status, w, h, pixels RGB or None, coefficients, planes)"""
    pack, out = str(tmp_path / "pack.bin"), str(tmp_path / "out.bin")
    off = np.zeros(len(streams) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in streams])
    with open(pack, "wb") as fh:
        fh.write(struct.pack("<q", len(streams)) + off.tobytes() + b"".join(streams))
    run = subprocess.run([exe, pack, out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and f"jpeg rules ok {len(streams)}, headers equal on 1 and 4 parts" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    raw = open(out, "rb").read()
    res, p = [], 0
    for _ in streams:
        st, w, h, nc, npl = struct.unpack_from("<iiiqq", raw, p)
        p += 28
        if st:
            res.append((st, w, h, None, None, None))
            continue
        px = np.frombuffer(raw, np.uint8, w * h * 3, p).reshape(h, w, 3)
        p += w * h * 3
        coef = np.frombuffer(raw, np.int16, nc, p)
        p += 2 * nc
        planes = np.frombuffer(raw, np.uint8, npl, p)
        p += npl
        res.append((st, w, h, px, coef, planes))
    assert p == len(raw)
    return res


def _ref(data):
    """the restatement on one stream -> (status, pixels, coefficients, planes)"""
    try:
        h, coef, pl, px = R.decode_all(data, "RGB")
    except R.JpegError:
        return E_IO, None, None, None
    return 0, px, np.concatenate([c.reshape(-1) for c in coef]), np.concatenate([p.reshape(-1) for p in pl])


def _same(got, data, what):
    st, px, coef, planes = _ref(data)
    assert got[0] == st, f"{what}: status {got[0]}, the restatement {st}"
    if st == 0:
        assert np.array_equal(got[4], coef), f"{what}: coefficients"
        assert np.array_equal(got[5], planes), f"{what}: planes"
        assert np.array_equal(got[3], px), f"{what}: pixels"
    return st


def test_the_shared_rules_equal_the_restatement(tmp_path):
    """coefficients, planes and pixels of every accepted fixture: exactly the restatement's; the rejected ones: MVS_E_IO"""
    exe = _build(tmp_path, False)
    names = ACCEPTED + sorted(REJECTED)
    res = _run(exe, tmp_path, [FIX[k][0] for k in names])
    for name, got in zip(names, res):
        st = _same(got, FIX[name][0], name)
        assert st == (0 if name in ACCEPTED else E_IO)
        if st == 0:
            assert np.array_equal(got[3], FIX[name][1]), name


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """the program, not a library loaded into Python, under ASan and UBSan: every accepted fixture; the 8x9 4:2:0 file truncated at every
    length; 200 seeded single-byte corruptions of the 17x23 4:2:0 file; the scan-error stream of the GPU tests.  Every run ends with a
    status and no report, and where the status is MVS_OK the pixels are the restatement's on the same bytes"""
    exe = _build(tmp_path, True)
    small, mid = FIX["8x9_420_q50"][0], FIX["17x23_420_q50"][0]
    rng = np.random.default_rng(27)
    streams = [FIX[k][0] for k in ACCEPTED] + [small[:n] for n in range(len(small))]
    for _ in range(200):
        b = bytearray(mid)
        b[int(rng.integers(len(b)))] = int(rng.integers(256))
        streams.append(bytes(b))
    streams.append(cut_scan(FIX["33x50_420_q50"][0]))
    res = _run(exe, tmp_path, streams)
    counts = {0: 0, E_IO: 0}
    for i, (got, data) in enumerate(zip(res, streams)):
        counts[_same(got, data, f"stream {i}")] += 1
    print("statuses:", counts)
    assert res[-1][0] == E_IO and all(r[0] == 0 for r in res[:len(ACCEPTED)])
    assert counts[0] > len(ACCEPTED) + 20 and counts[E_IO] > len(small) // 2       # both outcomes occur among the damaged streams


# ------------------------------------------------------------------ the host entries ----
def test_info_and_the_entries_without_a_device():
    from multiviewstitch_amd import _lib as L, processor as P
    lib = L.lib()
    for name in ("mvs_jpeg_info", "mvs_jpeg_decode", "mvs_jpeg_decode_dev", "mvs_processor_load_images", "mvs_processor_refine_depths_files"):
        assert hasattr(lib, name) and name in L.EXPORTS
    for name in ACCEPTED:
        assert P.JpegInfo(FIX[name][0]) == R.info(FIX[name][0]), name
    for name, word in REJECTED.items():
        with pytest.raises(L.MvsError) as e:
            P.JpegInfo(FIX[name][0])
        assert e.value.code == E_IO and word in str(e.value) and "image 0" in str(e.value)
    data = FIX["8x9_420_q50"][0]
    for n in range(len(data)):                                       # the walk reads nothing past len: a status for every length
        buf = np.frombuffer(data[:n] or b"\0", np.uint8).copy()
        info = L.CJpegInfo()
        assert lib.mvs_jpeg_info(L.ptr(buf), n, C.byref(info)) in (0, E_IO)
    if L.device_count() == 0:
        with pytest.raises(L.MvsError) as e:
            P.DecodeJpegs([data])
        assert e.value.code == E_NO_DEVICE
    with pytest.raises(L.MvsError) as e:                             # a rejected stream is reported with or without a device
        P.DecodeJpegs([data, FIX["17x23_progressive"][0]])
    assert e.value.code == E_IO and "image 1" in str(e.value) and "progressive" in str(e.value)
