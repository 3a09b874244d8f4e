"""mvs_jpeg_decode on the GPU (csrc/jpeg.hip) against the pixels Pillow decoded from the streams of tests/golden/jpeg, byte for byte:
every fixture alone in both channel orders, the 33x50 streams of every mode, table set and restart form in one call, more segments than a
workgroup has waves, the 1x1 files, run-to-run identity, the device form on a stream, the errors, and the directory chain LoadImages ->
LoadSequenceFiles / RefineDepthFilesFromJpeg.  No test here imports Pillow."""
import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P
from tests.test_jpeg_host import ACCEPTED, FIX, cut_scan

pytestmark = pytest.mark.gpu
E_INVALID, E_IO = -1, -10
MIXED = sorted(k for k in ACCEPTED if k.startswith("33x50_"))


@pytest.mark.parametrize("name", ACCEPTED)
def test_every_fixture_alone_in_both_orders(name):
    data, px = FIX[name]
    bgr, rgb = P.DecodeJpegs([data]), P.DecodeJpegs([data], order="RGB")
    print(name, int((rgb[0] != px).sum()), "differing bytes")
    assert rgb.dtype == np.uint8 and rgb.shape == (1,) + px.shape
    assert np.array_equal(rgb[0], px) and np.array_equal(bgr[0], px[..., ::-1])


def test_the_33x50_streams_mixed_in_one_call_and_two_runs():
    """all modes, qualities, custom tables, restart forms, SOF1 and 16-bit quantisers in one call: a table or offset of the wrong image shows"""
    assert len(MIXED) == 14                                          # the 8 of the size matrix and the 6 variants; two of them once more: 16 streams
    names = MIXED + MIXED[:2]
    a = P.DecodeJpegs([FIX[k][0] for k in names], order="RGB")
    for i, k in enumerate(names):
        assert np.array_equal(a[i], FIX[k][1]), (i, k, int((a[i] != FIX[k][1]).sum()))
    b = P.DecodeJpegs([FIX[k][0] for k in names], order="RGB")
    assert a.tobytes() == b.tobytes()


def test_more_segments_than_a_workgroup_has_waves():
    two = ["17x23_420_q50", "17x23_grey_q95"]
    a = P.DecodeJpegs([FIX[two[i % 2]][0] for i in range(140)])
    for i in range(140):
        assert np.array_equal(a[i], FIX[two[i % 2]][1][..., ::-1]), i
    for k in ("75x100_420_rst1", "75x100_444_rst1"):
        assert P.JpegInfo(FIX[k][0])["n_segments"] in (35, 130)
        assert np.array_equal(P.DecodeJpegs([FIX[k][0]], order="RGB")[0], FIX[k][1]), k


def test_the_1x1_files_in_one_call():
    names = sorted(k for k in ACCEPTED if k.startswith("1x1_"))
    assert len(names) == 8
    a = P.DecodeJpegs([FIX[k][0] for k in names], order="RGB")
    for i, k in enumerate(names):
        assert np.array_equal(a[i], FIX[k][1]), k


def test_the_device_form_on_a_stream_writes_the_same_bytes():
    import torch
    s = torch.cuda.Stream()
    t = P.DecodeJpegs([FIX[k][0] for k in MIXED], order="RGB", device="cuda", stream=s.cuda_stream)
    assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (len(MIXED), 33, 50, 3)
    host = t.cpu().numpy()                                           # the entry returns with the work complete
    for i, k in enumerate(MIXED):
        assert np.array_equal(host[i], FIX[k][1]), k
    t0 = P.DecodeJpegs([FIX[k][0] for k in MIXED], order="RGB", device="cuda")
    assert torch.equal(t, t0)


def test_the_timed_hook_writes_the_bytes_of_the_plain_entry():
    """mvs_test_jpeg_decode_timed on the sixteen 33x50 streams against mvs_jpeg_decode_dev, and the plain entry once more after it"""
    import ctypes as C
    import torch
    lib = L.lib()
    datas = [FIX[k][0] for k in MIXED + MIXED[:2]]

    def call(datas, ms):
        off = np.zeros(len(datas) + 1, np.int64)
        off[1:] = np.cumsum([len(d) for d in datas])
        blob = np.frombuffer(b"".join(datas), np.uint8)
        out = torch.zeros((len(datas), 33, 50, 3), dtype=torch.uint8, device="cuda")
        if ms is None:
            rc = lib.mvs_jpeg_decode_dev(len(datas), L.ptr(off), L.ptr(blob), L.JPEG_RGB, L.ptr(out), None)
        else:
            rc = lib.mvs_test_jpeg_decode_timed(len(datas), L.ptr(off), L.ptr(blob), L.JPEG_RGB, L.ptr(out), None, ms)
        return rc, out.cpu().numpy()

    rc, want = call(datas, None)
    assert rc == 0
    ms = (C.c_double * 5)(-1.0, -1.0, -1.0, -1.0, -1.0)
    rc, got = call(datas, ms)
    print("ms", list(ms))
    assert rc == 0 and np.array_equal(got, want)
    assert all(np.isfinite(m) and m >= 0 for m in ms)
    rc, again = call(datas, None)
    assert rc == 0 and np.array_equal(again, want)


def test_errors():
    with pytest.raises(L.MvsError) as e:
        P.DecodeJpegs([FIX["33x50_420_q50"][0], FIX["17x23_420_q50"][0], FIX["33x50_444_q50"][0]])
    assert e.value.code == E_INVALID and "image 1" in str(e.value)
    with pytest.raises(L.MvsError) as e:
        P.DecodeJpegs([FIX["33x50_420_q50"][0], FIX["33x50_444_q50"][0], FIX["17x23_progressive"][0]])
    assert e.value.code == E_IO and "image 2" in str(e.value) and "progressive" in str(e.value)


def test_a_scan_that_ends_early_fails_the_call():
    """the one malformed stream that runs on the GPU: tests/test_jpeg_host.py decodes these exact bytes under the sanitizers first"""
    good = FIX["33x50_444_q50"][0]
    with pytest.raises(L.MvsError) as e:
        P.DecodeJpegs([good, cut_scan(FIX["33x50_420_q50"][0]), good])
    assert e.value.code == E_IO and "image 1" in str(e.value) and "scan" in str(e.value)


# ------------------------------------------------------------------ the directory chain ----
def _cameras(n, shift):
    cams = []
    for i in range(n):
        c = L.CCamera()
        c.fx, c.fy, c.cx, c.cy, c.w, c.h = 60.0, 60.0, 25.0, 16.5, 50, 33
        c.R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        c.t[:] = [0.05 * i + shift, 0.0, 0.0]
        cams.append(c)
    return cams


def _sequences(tmp_path):
    names = (["33x50_444_q95", "33x50_420_q95", "33x50_422_q95"], ["33x50_420_opt", "33x50_grey_q95", "33x50_420_rstrow"])
    cameras = [_cameras(3, 0.0), _cameras(3, 0.02)]
    rng = np.random.default_rng(5)
    dirs, depths = [], []
    for k, seq in enumerate(names):
        d = tmp_path / f"seq{k}"
        for sub in ("Render", "CHECK"):
            (d / "DATA" / sub).mkdir(parents=True)
        ras = (0.1 + 0.01 * rng.random((3, 33, 50))).astype(np.float32)
        for i, name in enumerate(seq):
            (d / f"{i:05d}.jpg").write_bytes(FIX[name][0])
            for sub in ("Render", "CHECK"):
                IO.SaveDepth(str(d / "DATA" / sub / f"_depth{i}.raw"), ras[i])
        dirs.append(str(d) if k else str(d) + "/")                   # with and without the trailing '/'
        depths.append(ras)
    rgb = [np.stack([FIX[n][1] for n in seq]) for seq in names]
    return dirs, cameras, depths, rgb


def test_load_images_equals_the_goldens(tmp_path):
    dirs, cameras, _, rgb = _sequences(tmp_path)
    for order, want in (("RGB", rgb), ("BGR", [a[..., ::-1] for a in rgb])):
        got = P.LoadImages(dirs, cameras, order)
        assert len(got) == 2 and all(np.array_equal(g, w) for g, w in zip(got, want))
    (tmp_path / "seq1" / "00002.jpg").unlink()
    with pytest.raises(L.MvsError) as e:
        P.LoadImages(dirs, cameras)
    assert e.value.code == E_IO and "00002.jpg" in str(e.value)


def test_load_sequence_files_equals_load_sequence_models(tmp_path):
    dirs, cameras, depths, rgb = _sequences(tmp_path)
    got = P.LoadSequenceFiles(dirs[0], cameras[0], 2, 1, 0.1)
    want = P.LoadSequenceModels(cameras[0], np.ascontiguousarray(rgb[0][..., ::-1]), depths[0], 2, 1, 0.1)
    assert sorted(got) == sorted(want)
    for key in want:
        if key == "cameras":
            assert got[key] == want[key]
        else:
            assert np.array_equal(got[key], want[key]), key


def test_refine_from_jpeg_writes_what_refine_files_writes(tmp_path):
    dirs, cameras, _, rgb = _sequences(tmp_path)
    P.RefineDepthFilesFromJpeg(dirs, cameras)
    mine = [[(tmp_path / f"seq{k}" / "DATA" / "Refine" / f"_depth{i}.raw").read_bytes() for i in range(3)] for k in range(2)]
    for k in range(2):
        for i in range(3):
            (tmp_path / f"seq{k}" / "DATA" / "Refine" / f"_depth{i}.raw").unlink()
    P.RefineDepthFiles(dirs, cameras, rgb)
    for k in range(2):
        for i in range(3):
            assert len(mine[k][i]) == 33 * 50 * 4
            assert (tmp_path / f"seq{k}" / "DATA" / "Refine" / f"_depth{i}.raw").read_bytes() == mine[k][i]
