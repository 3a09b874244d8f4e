"""The GPU-only parts of the JPEG codec on the coefficient cases of tests/jpeg_coef_cases.py: the encoder's bit writer, FF count, scans,
stuffing and marker placement (csrc/jpeg_enc.hip behind its transform, through ``mvs_test_jpeg_encode_coef``) against
``ref_jpeg_enc.encode_coef`` byte for byte and offset for offset, and the decoder's byte ring and slow Huffman path (csrc/jpeg.hip) on those
streams against ``ref_jpeg.decode`` and, where tests/golden/jpeg_coef holds them, Pillow's pixels.  tests/test_jpeg_coef_host.py shows on the
CPU that the cases reach FF-dense buffers, FF at chunk boundaries and interval ends, every symbol of both tables, segments of many ring
windows and the longest block.  Every input is valid.  No test here imports Pillow."""
import ctypes as C

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import jpeg_coef_cases as K, ref_jpeg_enc as E
from tests.make_jpeg_coef_golden import load_all
from tests.test_jpeg_host import FIX as NATURAL

pytestmark = pytest.mark.gpu
E_INVALID = -1
FIX = load_all()
NAMES = list(K.CASES)


def encode_coef(images, w, h, mode, quality=100, restart=0, capacity=None):
    """mvs_test_jpeg_encode_coef on the coefficient arrays of n images -> (status, streams, offsets as the call wrote them)"""
    lib = L.lib()
    n = len(images)
    flags = L.JPEG_GREY if mode == "grey" else 0
    prm = P.jpeg_encode_params(quality=quality, sampling=420 if mode == "grey" else int(mode), restart_interval=restart)
    coef = np.ascontiguousarray(np.concatenate([K.flat(a) for a in images]))
    cap = n * int(L.check(lib.mvs_jpeg_encode_bound(w, h, flags, C.byref(prm)))) if capacity is None else capacity
    off, out = np.full(n + 1, -1, np.int64), np.zeros(max(1, cap), np.uint8)
    rc = lib.mvs_test_jpeg_encode_coef(n, w, h, L.ptr(coef), flags, C.byref(prm), L.ptr(off), L.ptr(out), cap)
    return rc, [out[off[i]:off[i + 1]].tobytes() for i in range(n)] if rc == 0 else None, off


def same_streams(got, off, want, what):
    assert off.tolist() == np.cumsum([0] + [len(s) for s in want]).tolist(), what
    for i, (g, s) in enumerate(zip(got, want)):
        if g != s:
            first = next((k for k in range(min(len(g), len(s))) if g[k] != s[k]), min(len(g), len(s)))
            raise AssertionError(f"{what}, image {i}: {len(g)} bytes for {len(s)}, the first difference at byte {first}")


@pytest.mark.parametrize("name", NAMES)
def test_every_case_alone_equals_the_restatement(name):
    c = K.CASES[name]
    want = K.encoded(name)[0]
    rc, got, off = encode_coef([K.coef(name)], c["w"], c["h"], c["mode"], c["quality"], c["restart"])
    assert rc == 0, L.lib().mvs_last_error().decode()
    print(name, len(got[0]), "bytes, the restatement", len(want))
    same_streams(got, off, [want], name)


GROUPS = {"33x50_444": (33, 50, "444", ["ff_33x50_444", "zrl_33x50_444", "rand_33x50_444", "max_33x50_444_rst2"]),
          "17x23_422": (17, 23, "422", ["ff_17x23_422", "sym_17x23_422", "zrl_17x23_422", "rand_17x23_422", "max_17x23_422"]),
          "17x23_420": (17, 23, "420", ["rand_17x23_420", "max_17x23_420", "ff_17x23_420_rstrow", "sym_17x23_420_rstrow", "zrl_17x23_420_rstrow"]),
          "33x50_grey": (33, 50, "grey", ["ff_33x50_grey", "zrl_33x50_grey", "rand_33x50_grey", "rand_33x50_grey_rst2"])}


@pytest.mark.parametrize("restart", [0, 1, 2, K.ROW])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_different_cases_of_one_size_in_one_call_and_two_runs(group, restart):
    """the coefficients of four or five cases of one size and mode as the images of one call, under every restart form: an offset, a DC
    predecessor or an interval of the wrong image shows; the second run writes the same bytes"""
    h, w, mode, names = GROUPS[group]
    images = [K.coef(n) for n in names]
    want = [E.encode_coef(a, w, h, mode, 100, restart)[0] for a in images]
    rc, got, off = encode_coef(images, w, h, mode, 100, restart)
    assert rc == 0, L.lib().mvs_last_error().decode()
    same_streams(got, off, want, f"{group} restart {restart}")
    rc, again, off2 = encode_coef(images, w, h, mode, 100, restart)
    assert rc == 0 and again == got and np.array_equal(off, off2)


def test_the_chunk_boundary_call():
    """FF on both sides of a 1024-byte boundary of the call-wide unstuffed buffer and an FF in its last partial dword
    (test_jpeg_coef_host.py asserts both on the restatement's bytes)"""
    images, raw = K.boundary_call()
    assert K.boundary_figures(raw)[0] and K.boundary_figures(raw)[1]
    want = [E.encode_coef(a, 50, 33, "444", 100, 0)[0] for a in images]
    rc, got, off = encode_coef(images, 50, 33, "444")
    assert rc == 0, L.lib().mvs_last_error().decode()
    same_streams(got, off, want, "the chunk-boundary call")


def test_a_capacity_one_byte_short_still_writes_offsets():
    h, w, mode, names = GROUPS["33x50_444"]
    images = [K.coef(n) for n in names]
    want = [E.encode_coef(a, w, h, mode, 100, 0)[0] for a in images]
    total = sum(len(s) for s in want)
    rc, got, off = encode_coef(images, w, h, mode, capacity=total)
    assert rc == 0 and got == want
    rc, _, off = encode_coef(images, w, h, mode, capacity=total - 1)
    assert rc == E_INVALID and "capacity" in L.lib().mvs_last_error().decode()
    assert off.tolist() == np.cumsum([0] + [len(s) for s in want]).tolist()


# ------------------------------------------------------------------ the decoder on these streams ----
@pytest.mark.parametrize("name", NAMES)
def test_decode_every_stream_alone_in_both_orders(name):
    """``long`` among them: one segment of more than eight windows of the byte ring"""
    data, want = K.encoded(name)[0], K.decoded(name)[3]
    rgb, bgr = P.DecodeJpegs([data], order="RGB"), P.DecodeJpegs([data])
    print(name, len(data), "bytes,", int((rgb[0] != want).sum()), "differing bytes")
    assert rgb.dtype == np.uint8 and rgb.shape == (1,) + want.shape
    assert np.array_equal(rgb[0], want) and np.array_equal(bgr[0], want[..., ::-1])
    if name in FIX:
        assert np.array_equal(rgb[0], FIX[name][1])                 # what Pillow decoded


MIXED = ["ff_33x50_444", "33x50_444_q95", "rand_33x50_444", "zrl_33x50_444", "max_33x50_444_rst2", "33x50_444_q50", "ff_33x50_444_rst2"]


def _mixed():
    """-> (streams, R G B pixels): FF-dense, natural, random, sparse and longest-block streams of one size and mode"""
    datas = [NATURAL[k][0] if k in NATURAL else K.encoded(k)[0] for k in MIXED]
    return datas, [NATURAL[k][1] if k in NATURAL else K.decoded(k)[3] for k in MIXED]


def test_decode_a_call_that_mixes_dense_natural_and_random_streams():
    datas, want = _mixed()
    assert any(k in NATURAL for k in MIXED) and np.array_equal(FIX["ff_33x50_444"][1], want[0])
    for order in ("RGB", "BGR"):
        a = P.DecodeJpegs(datas, order=order)
        for i, k in enumerate(MIXED):
            px = want[i] if order == "RGB" else want[i][..., ::-1]
            assert np.array_equal(a[i], px), (order, i, k, int((a[i] != px).sum()))
    assert P.DecodeJpegs(datas, order="RGB").tobytes() == P.DecodeJpegs(datas, order="RGB").tobytes()


def test_decode_the_device_form_on_a_stream():
    import torch
    datas, want = _mixed()
    s = torch.cuda.Stream()
    t = P.DecodeJpegs(datas, order="RGB", device="cuda", stream=s.cuda_stream)
    assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (len(MIXED), 33, 50, 3)
    host = t.cpu().numpy()                                           # the entry returns with the work complete
    for i, k in enumerate(MIXED):
        assert np.array_equal(host[i], want[i]), k
    data = K.encoded("long_75x100_444")[0]
    t = P.DecodeJpegs([data], order="RGB", device="cuda", stream=s.cuda_stream)
    assert np.array_equal(t.cpu().numpy()[0], K.decoded("long_75x100_444")[3])


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_decode_what_the_gpu_encoded(group):
    """the streams of mvs_test_jpeg_encode_coef through DecodeJpegs: the pixels of the restatement's streams through DecodeJpegs, and the
    restatement's pixels"""
    h, w, mode, names = GROUPS[group]
    images = [K.coef(n) for n in names]
    rc, got, _ = encode_coef(images, w, h, mode, 100, 2)
    assert rc == 0, L.lib().mvs_last_error().decode()
    want = [E.encode_coef(a, w, h, mode, 100, 2)[0] for a in images]
    a, b = P.DecodeJpegs(got, order="RGB"), P.DecodeJpegs(want, order="RGB")
    assert np.array_equal(a, b)
    for i, n in enumerate(names):                                    # the restart interval changes the stream, not the pixels
        assert np.array_equal(a[i], K.decoded(n)[3]), n
