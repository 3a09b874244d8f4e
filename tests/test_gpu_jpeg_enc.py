"""mvs_jpeg_encode, mvs_jpeg_roundtrip and mvs_depth_preview on the GPU (csrc/jpeg_enc.hip) against the streams Pillow wrote for the inputs of
tests/golden/jpeg_enc and against the restatement tests/ref_jpeg_enc.py, byte for byte: every fixture alone in both channel orders, 16
images of one parameter set in one call, 140 images in one call, 130 restart intervals, the 1x1 inputs, the capacity rule, the device
form on a stream, the round trip, the views of LoadSequenceModels, and the file forms.  No test here imports Pillow."""
import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P
from tests import ref_jpeg_enc as E
from tests.make_jpeg_golden import image
from tests.test_jpeg_enc_host import FIX, NAMES

pytestmark = pytest.mark.gpu
E_INVALID = -1


def _args(f):
    """the keywords of EncodeJpegs for a fixture, its pixels as R G B or grey"""
    grey = f["mode"] == "grey"
    return dict(quality=f["quality"], sampling="420" if grey else f["mode"], restart_interval=f["restart"], order="GREY" if grey else "RGB")


@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_alone_in_both_orders(name):
    f = FIX[name]
    kw = _args(f)
    (got,) = P.EncodeJpegs(f["pixels"][None], **kw)
    print(name, len(got), "bytes, golden", len(f["jpg"]))
    assert got == f["jpg"]
    if f["mode"] != "grey":
        kw["order"] = "BGR"
        (got,) = P.EncodeJpegs(np.ascontiguousarray(f["pixels"][None, ..., ::-1]), **kw)
        assert got == f["jpg"]


def test_sixteen_images_of_one_parameter_set_and_two_runs():
    """one call has one parameter set: 16 different 33x50 inputs at 4:2:0, quality 75, interval 2, against the restatement"""
    imgs = np.stack([FIX["33x50_420_q95"]["pixels"]] + [image(33, 50, seed) for seed in range(1, 16)])
    a = P.EncodeJpegs(imgs, quality=75, sampling="420", restart_interval=2, order="RGB")
    assert a[0] == FIX["33x50_420_rst2"]["jpg"]
    for i in range(16):
        assert a[i] == E.encode(imgs[i], "420", 75, 2), i
    assert a == P.EncodeJpegs(imgs, quality=75, sampling="420", restart_interval=2, order="RGB")


def test_140_images_in_one_call():
    two = [FIX["17x23_420_q50"], FIX["17x23_444_q50"]]
    imgs = np.stack([two[i % 2]["pixels"] for i in range(140)])
    a = P.EncodeJpegs(imgs, quality=50, sampling="420", order="RGB")
    want = [FIX["17x23_420_q50"]["jpg"], E.encode(two[1]["pixels"], "420", 50)]
    for i in range(140):
        assert a[i] == want[i % 2], i


def test_130_intervals_and_one_row_per_interval():
    f = FIX["75x100_444_rst1"]
    assert P.EncodeJpegs(f["pixels"][None], **_args(f)) == [f["jpg"]]
    assert P.JpegInfo(f["jpg"])["n_segments"] == 130
    g = FIX["33x50_420_rstrow"]
    assert P.EncodeJpegs(g["pixels"][None], quality=75, restart_interval=L.JPEG_RESTART_ROW, order="RGB") == [g["jpg"]]


def test_1x1_in_all_modes():
    for name in sorted(k for k in NAMES if k.startswith("1x1_")):
        f = FIX[name]
        assert P.EncodeJpegs(np.stack([f["pixels"]] * 3), **_args(f)) == [f["jpg"]] * 3, name


def test_capacity_one_byte_short():
    imgs = np.stack([image(33, 50, seed) for seed in range(4)])
    ok = P.EncodeJpegs(imgs, quality=75, order="RGB")
    total = sum(len(s) for s in ok)
    assert P.EncodeJpegs(imgs, quality=75, order="RGB", capacity=total) == ok
    for device in (None, "cuda"):
        with pytest.raises(L.MvsError) as e:
            P.EncodeJpegs(imgs, quality=75, order="RGB", capacity=total - 1, device=device)
        assert e.value.code == E_INVALID
        assert e.value.offsets.tolist() == np.cumsum([0] + [len(s) for s in ok]).tolist()


def test_the_device_form_on_a_stream_equals_the_host_form():
    import torch
    imgs = np.stack([image(33, 50, seed) for seed in range(5)])
    host = P.EncodeJpegs(imgs, quality=95, sampling="422", restart_interval=3, order="BGR")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.as_tensor(imgs).to("cuda")
    data, off = P.EncodeJpegs(t, quality=95, sampling="422", restart_interval=3, order="BGR", device="cuda", stream=s.cuda_stream)
    assert data.is_cuda and data.dtype == torch.uint8 and off[0] == 0 and int(off[-1]) == data.numel()
    blob = data.cpu().numpy().tobytes()                              # the entry returns with the work complete
    assert [blob[off[i]:off[i + 1]] for i in range(5)] == host
    data0, off0 = P.EncodeJpegs(imgs, quality=95, sampling="422", restart_interval=3, order="BGR", device="cuda")
    assert torch.equal(data, data0) and np.array_equal(off, off0)


@pytest.mark.parametrize("restart", [0, 1])
def test_more_than_1024_scan_tiles_in_one_call(restart):
    """65535 copies of one 40 x 32 grey image, 20 blocks each: 1 310 700 scan blocks, 1280 tiles of the device-wide scan (csrc/scan_dev.h),
    the smallest call in which a thread of the scan's second level owns more than one tile sum; with an interval of one MCU the
    interval scan has 1 310 700 items as well.  Every stream is the stream of the image alone, which is the restatement's"""
    import torch
    n, img = 65535, image(40, 32, 7)[..., 1].copy()
    (one,) = P.EncodeJpegs(img[None], order="GREY", restart_interval=restart)
    assert one == E.encode(img, "grey", 95, restart)
    imgs = torch.as_tensor(img).to("cuda").expand(n, 40, 32).contiguous()
    data, off = P.EncodeJpegs(imgs, order="GREY", restart_interval=restart, device="cuda", capacity=n * len(one))
    print("restart", restart, len(one), "bytes per stream,", n * 20, "scan blocks,", -(-(n * 20 + 1) // 1024), "tiles")
    assert np.array_equal(off, np.arange(n + 1, dtype=np.int64) * len(one))
    row = torch.as_tensor(np.frombuffer(one, np.uint8).copy()).to("cuda")
    assert bool((data.view(n, len(one)) == row).all())


def test_the_timed_hook_writes_the_bytes_of_the_plain_entry():
    """mvs_test_jpeg_encode_timed on five 33x50 images against mvs_jpeg_encode_dev; then a capacity one byte short, which returns between
    the marks of the stage clock, and the plain entry after it"""
    import ctypes as C
    import torch
    lib = L.lib()
    imgs = torch.as_tensor(np.stack([image(33, 50, seed) for seed in range(5)])).to("cuda")
    prm = P.jpeg_encode_params(quality=75, sampling=420, restart_interval=2)
    cap = 5 * int(lib.mvs_jpeg_encode_bound(50, 33, L.JPEG_RGB, C.byref(prm)))

    def plain():
        off, data = np.zeros(6, np.int64), torch.zeros(cap, dtype=torch.uint8, device="cuda")
        L.check(lib.mvs_jpeg_encode_dev(5, 50, 33, L.ptr(imgs), L.JPEG_RGB, C.byref(prm), L.ptr(off), L.ptr(data), cap, None))
        return off, data[:int(off[5])].cpu().numpy()

    def timed(capacity):
        off, data, ms = np.zeros(6, np.int64), torch.zeros(cap, dtype=torch.uint8, device="cuda"), (C.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
        rc = lib.mvs_test_jpeg_encode_timed(5, 50, 33, L.ptr(imgs), L.JPEG_RGB, C.byref(prm), L.ptr(off), L.ptr(data), capacity, None, ms)
        return rc, off, data[:int(off[5])].cpu().numpy(), list(ms)

    off0, want = plain()
    rc, off, got, ms = timed(cap)
    print("ms", ms)
    assert rc == 0 and np.array_equal(off, off0) and np.array_equal(got, want)
    assert all(np.isfinite(m) and m >= 0 for m in ms)
    rc, off, _, _ = timed(int(off0[5]) - 1)
    assert rc == E_INVALID and np.array_equal(off, off0)
    off1, again = plain()
    assert np.array_equal(off1, off0) and np.array_equal(again, want)


@pytest.mark.parametrize("size", ["33x50", "8x9"])
@pytest.mark.parametrize("mode", ["grey", "444", "422", "420"])
def test_the_round_trip_equals_decode_of_encode(size, mode):
    f = FIX[f"{size}_{mode}_q95"]
    kw = _args(f)
    x = f["pixels"][None]
    got = P.JpegRoundTrip(x, **kw)
    order = "RGB" if mode == "grey" else kw["order"]
    assert got.dtype == np.uint8 and got.shape == x.shape[:3] + (3,)
    assert np.array_equal(got, P.DecodeJpegs(P.EncodeJpegs(x, **kw), order=order))
    want = f["decoded"] if mode != "grey" else np.stack([f["decoded"]] * 3, axis=2)
    assert np.array_equal(got[0], want)                              # what Pillow decoded from Pillow's stream
    if mode != "grey":
        kw["order"] = "BGR"
        assert np.array_equal(P.JpegRoundTrip(np.ascontiguousarray(x[..., ::-1]), **kw)[0], want[..., ::-1])
    import torch
    t = P.JpegRoundTrip(torch.as_tensor(x).to("cuda"), **_args(f))
    assert np.array_equal(t.cpu().numpy(), got)


def _cameras(n):
    cams = []
    for i in range(n):
        c = L.CCamera()
        c.fx, c.fy, c.cx, c.cy, c.w, c.h = 60.0, 60.0, 25.0, 16.5, 50, 33
        c.R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        c.t[:] = [0.05 * i, 0.0, 0.0]
        cams.append(c)
    return cams


def test_load_sequence_models_with_and_without_the_round_trip():
    cams = _cameras(3)
    imgs = np.stack([np.ascontiguousarray(image(33, 50, seed)[..., ::-1]) for seed in range(3)])
    depths = (0.1 + 0.01 * np.random.default_rng(5).random((3, 33, 50))).astype(np.float32)
    plain = P.LoadSequenceModels(cams, imgs, depths, 2, 1, 0.1)
    none = P.LoadSequenceModels(cams, imgs, depths, 2, 1, 0.1, jpeg_quality=None)
    assert sorted(plain) == sorted(none)
    for key in plain:
        assert plain[key] == none[key] if key == "cameras" else np.array_equal(plain[key], none[key]), key
    q95 = P.LoadSequenceModels(cams, imgs, depths, 2, 1, 0.1, jpeg_quality=95)
    v = plain["views"]
    assert np.array_equal(q95["views"], P.JpegRoundTrip(v.reshape((-1,) + v.shape[2:]), quality=95).reshape(v.shape))
    assert not np.array_equal(q95["views"], v) and np.array_equal(q95["tex"], plain["tex"])


RASTERS = np.stack([
    np.where(np.arange(33 * 50).reshape(33, 50) % 7 == 0, -1.0, 0.1 + 0.002 * np.arange(33 * 50).reshape(33, 50) % 0.37),   # negative pixels ...
    np.full((33, 50), 0.25),                                                                                                # constant
    np.full((33, 50), -1.0),                                                                                                # all invalid
]).astype(np.float32)
RASTERS[0, 3, 4:9] = np.nan                                                                                                # ... and NaN
RASTERS[2, 5, 5] = np.nan


def test_depth_preview_equals_the_restatement():
    got = P.DepthPreview(RASTERS)
    for i in range(3):
        assert np.array_equal(got[i], E.depth_preview(RASTERS[i])), i
    assert (got[1] == 0).all() and (got[2] == 255).all() and 0 < (got[0] == 255).sum() < got[0].size
    import torch
    assert np.array_equal(P.DepthPreview(torch.as_tensor(RASTERS).to("cuda")).cpu().numpy(), got)


def test_the_file_forms_write_what_encode_returns(tmp_path):
    d = tmp_path / "seq"
    for sub in ("CHECK", "Refine"):
        (d / "DATA" / sub).mkdir(parents=True)
        for i in range(3):
            IO.SaveDepth(str(d / "DATA" / sub / f"_depth{i}.raw"), RASTERS[i])
    want = P.EncodeJpegs(P.DepthPreview(RASTERS), order="GREY")
    P.DepthPreviewFiles(str(d) + "/", "CHECK", 3, 50, 33)
    P.DepthPreviewFiles(str(d), "Refine", 3, 50, 33)                 # with and without the trailing '/'
    for sub in ("CHECK", "Refine"):
        assert sorted(p.name for p in (d / "DATA" / sub).iterdir()) == sorted([f"_depth{i}.{e}" for i in range(3) for e in ("raw", "jpg")])
        for i in range(3):
            assert (d / "DATA" / sub / f"_depth{i}.jpg").read_bytes() == want[i], (sub, i)
    with pytest.raises(L.MvsError):
        P.DepthPreviewFiles(str(d), "Render", 3, 50, 33)             # no such rasters
    views = np.stack([image(33, 50, seed)[..., ::-1] for seed in range(6)]).reshape(3, 2, 33, 50, 3)
    P.SaveViews(str(d), views, quality=90)
    want = P.EncodeJpegs(views.reshape(6, 33, 50, 3), quality=90)
    assert sorted(p.name for p in (d / "Views").iterdir()) == sorted(f"proj{i}_{j}.jpg" for i in range(3) for j in range(2))
    for i in range(3):
        for j in range(2):
            assert (d / "Views" / f"proj{i}_{j}.jpg").read_bytes() == want[2 * i + j]
    assert np.array_equal(P.DecodeJpegs(want), P.JpegRoundTrip(views.reshape(6, 33, 50, 3), quality=90))
