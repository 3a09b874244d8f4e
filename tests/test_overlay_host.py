"""The overlay pictures without a GPU: the restatement tests/ref_overlay.py (rules O1-O6 of include/mvs.h) against a brute-force test with
exact rational distances, csrc/overlay_rules.h run as a host program of its own (tests/overlay_rules.cpp) against the restatement — plain,
and under the address and undefined-behaviour sanitizers —, mvs_cv_rng_colours through ctypes against the restatement's big-int generator,
and the argument checks of every new entry."""
import ctypes as C
import itertools
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import ref_overlay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -4
THICK = (1, 2, 3, 8)


# ------------------------------------------------------------------ the restatement against brute force ----
def brute_segment(w, h, a, b, T):
    """pixels within T / 2 of the segment a - b by the rational closest point: another formulation than O3's three cases"""
    out = np.zeros((h, w), bool)
    dx, dy = b[0] - a[0], b[1] - a[1]
    L2 = dx * dx + dy * dy
    for y in range(h):
        for x in range(w):
            t = Fraction(0) if L2 == 0 else min(Fraction(1), max(Fraction(0), Fraction((x - a[0]) * dx + (y - a[1]) * dy, L2)))
            qx, qy = a[0] + t * dx, a[1] + t * dy
            out[y, x] = 4 * ((x - qx) ** 2 + (y - qy) ** 2) <= T * T
    return out


def full_mask(p, w, h, exact=False):
    m = np.zeros((h, w), bool)
    ys, xs, sub = R.mask(p, w, h, exact)
    m[ys, xs] = sub
    return m


def test_segments_equal_the_rational_brute_force():
    w, h = 24, 19
    ends = [(0, 0), (23, 18), (23, 0), (0, 18), (5, 7), (6, 7), (5, 12), (17, 3), (11, 11), (12, 18)]
    n = 0
    for a, b in itertools.product(ends, ends):
        for T in THICK:
            p = R.prim(R.SEGMENT, a[0], a[1], b[0], b[1], T)
            want = brute_segment(w, h, a, b, T)
            assert np.array_equal(full_mask(p, w, h), want), (a, b, T)
            assert np.array_equal(full_mask(p, w, h, exact=True), want), (a, b, T)
            assert all(R.covers(p, x, y) == want[y, x] for y in range(h) for x in range(0, w, 5))
            n += 1
    assert n == 400


def test_radius_one_is_the_plus_and_its_four_neighbours():
    plus = {(5, 4), (4, 5), (5, 5), (6, 5), (5, 6)}
    disc = full_mask(R.prim(R.DISC, 5, 5, size=1), 11, 11)
    ring = full_mask(R.prim(R.RING, 5, 5, size=1), 11, 11)
    assert {(x, y) for y, x in zip(*np.nonzero(disc))} == plus
    assert {(x, y) for y, x in zip(*np.nonzero(ring))} == plus - {(5, 5)}
    assert {(x, y) for y, x in zip(*np.nonzero(full_mask(R.prim(R.RING, 5, 5, size=0), 11, 11)))} == {(5, 5)}
    assert {(x, y) for y, x in zip(*np.nonzero(full_mask(R.prim(R.DISC, 5, 5, size=0), 11, 11)))} == {(5, 5)}
    for r in (2, 3, 7):                                               # a disc is its rings
        rings = sum(full_mask(R.prim(R.RING, 9, 8, size=k), 24, 24).astype(int) for k in range(r + 1))
        assert np.array_equal(rings, full_mask(R.prim(R.DISC, 9, 8, size=r), 24, 24).astype(int))
    assert full_mask(R.prim(R.DISC, -1, 3, size=1), 8, 8).sum() == 1 and full_mask(R.prim(R.DISC, -2, 3, size=1), 8, 8).sum() == 0


def test_cv_round_is_half_to_even():
    got = [R.cv_round(v) for v in (2.5, 3.5, -0.5, -1.5, 0.49999997, 7.0, float("nan"), float("inf"), 3e9, -3e9)]
    assert got == [2, 4, 0, -2, 0, 7, R.INT_MIN, R.INT_MIN, R.INT_MIN, R.INT_MIN]


# ------------------------------------------------------------------ the shared rules as a program ----
def _build(tmp_path, sanitize):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / ("overlay_rules_san" if sanitize else "overlay_rules"))
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "overlay_rules.cpp"), "-o", exe])
    return exe


def pack_prims(prims):
    from multiviewstitch_amd import _lib as L
    return np.array(prims, dtype=L.DRAW_PRIM_DTYPE).reshape(-1).tobytes()


def cases():
    """-> [(what, canvas [h, w, 3], prims)]: ragged tiles, every kind at the corners and clipped from outside, segments of every slope and
    thickness, an order case of 300 overlapping primitives, large radii (the ring's hole), and the widest canvas with the thickest line"""
    rng = np.random.default_rng(30)
    out = []
    w, h = 37, 29
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    corners = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    col = lambda: tuple(int(c) for c in rng.integers(0, 256, 3))
    for kind in (R.DISC, R.RING):
        for r in (0, 1, 2, 5):
            out.append((f"kind{kind}_r{r}_corners", base, [R.prim(kind, x, y, size=r, colour=col()) for x, y in corners]))
        out.append((f"kind{kind}_outside", base, [R.prim(kind, x, y, size=r, colour=col())
                                                 for x, y, r in ((-1, 5, 1), (-2, 5, 1), (w, 9, 1), (18, -3, 6), (40, 33, 9), (-2 ** 20, 2 ** 20, 255),
                                                                 (18, 14, 40), (18, 14, 255), (-100, 14, 120))]))
    segs = [((3, 9), (33, 9)), ((20, 2), (20, 27)), ((4, 3), (26, 25)), ((15, 1), (18, 27)), ((1, 12), (35, 15)), ((22, 17), (22, 17)),
            ((0, 0), (w - 1, h - 1)), ((w - 1, 0), (0, h - 1))] + [(c, c) for c in corners]
    for T in THICK:
        out.append((f"segments_T{T}", base, [R.prim(R.SEGMENT, a[0], a[1], b[0], b[1], T, col()) for a, b in segs]))
    many = []                                                         # 44 large ones, then 256 small ones that leave some of them visible
    for k in range(300):
        kind = (R.DISC, R.RING, R.SEGMENT)[k % 3]
        x0, y0, x1, y1 = (int(v) for v in rng.integers(0, (w, h, w, h)))
        if k >= 44:
            x1, y1 = int(np.clip(x0 + rng.integers(-6, 7), 0, w - 1)), int(np.clip(y0 + rng.integers(-6, 7), 0, h - 1))
        many.append(R.prim(kind, x0, y0, x1, y1, int(rng.integers(1, 9 if k < 44 else 3)), (k % 256, k // 256, 255 - k % 251)))
    cover = R.prim(R.DISC, 18, 14, size=60, colour=(1, 2, 3))
    out += [("order_300", base, many), ("order_cover_last", base, many + [cover]), ("order_cover_first", base, [cover] + many)]
    out.append(("empty", base, []))
    wide = rng.integers(0, 256, (8, 16384, 3), dtype=np.uint8)
    out.append(("wide_T255", wide, [R.prim(R.SEGMENT, 0, 0, 16383, 7, 255, (9, 8, 7))]))
    out.append(("wide_T3", wide, [R.prim(R.SEGMENT, 0, 0, 16383, 7, 3, (9, 8, 7))]))
    out.append(("diagonal_512", np.zeros((512, 512, 3), np.uint8), [R.prim(R.SEGMENT, 0, 0, 511, 511, 2, (7, 8, 9))]))
    return out


_WANT = {}


def want(what, canvas, prims):
    """the restatement on a case, computed once (Python integers where the int64 bound is the point)"""
    if what not in _WANT:
        _WANT[what] = R.draw(canvas, prims, exact=what.startswith("wide"))
    return _WANT[what]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_shared_rules_equal_the_restatement(tmp_path, sanitize):
    """the program, not a library loaded into Python: canvases, roundings, colours and match primitives are the restatement's, no
    covering primitive is dropped by the tile test (the program aborts on one), and the sanitized build ends without a report"""
    cs = cases()
    floats = np.array([2.5, 3.5, -0.5, -1.5, 0.49999997, 36.6, -0.4, np.nan, np.inf, -np.inf, 3e9, -3e9, 2147483520.0, -2147483648.0, 1e-40],
                      np.float32)
    rng = np.random.default_rng(6)
    matches = rng.integers(0, 24, (17, 4)).astype(np.int32)
    state0, state1 = 0x123456789ABCDEF0, R.RNG_DEFAULT
    pack, outp = str(tmp_path / "pack.bin"), str(tmp_path / "out.bin")
    with open(pack, "wb") as fh:
        fh.write(struct.pack("<q", len(cs)))
        for _, canvas, prims in cs:
            fh.write(struct.pack("<3i", canvas.shape[1], canvas.shape[0], len(prims)))
            fh.write(pack_prims(prims))
            fh.write(np.ascontiguousarray(canvas).tobytes())
        fh.write(struct.pack("<q", len(floats)) + floats.tobytes())
        fh.write(struct.pack("<Qq", state0, 40))
        fh.write(struct.pack("<2iq", 24, 1, len(matches)) + matches.tobytes() + struct.pack("<Q", state1))
    run = subprocess.run([_build(tmp_path, sanitize), pack, outp], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and f"overlay rules ok {len(cs)}" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    raw, p = open(outp, "rb").read(), 0
    for what, canvas, prims in cs:
        got = np.frombuffer(raw, np.uint8, canvas.size, p).reshape(canvas.shape)
        p += canvas.size
        survivors, tiles = struct.unpack_from("<2q", raw, p)
        p += 16
        print(what, "survivors per tile", survivors / tiles)
        assert np.array_equal(got, want(what, canvas, prims)), what
        if what == "diagonal_512":                                    # the tile test is tight: a band of at most three tiles per tile
            assert tiles == 1024 and 32 <= survivors <= 3 * 32        # row along the line, not the 1024 tiles of its bounding box
    assert np.frombuffer(raw, np.int32, len(floats), p).tolist() == [R.cv_round(v) for v in floats]
    p += 4 * len(floats)
    g = R.Rng(state0)
    assert np.frombuffer(raw, np.uint8, 120, p).reshape(40, 3).tolist() == [list(g.colour()) for _ in range(40)]
    assert struct.unpack_from("<Q", raw, p + 120)[0] == g.state
    p += 128
    g = R.Rng(state1)
    assert raw[p:p + 24 * 51] == pack_prims(R.match_prims(matches, 24, g, swap=True))
    assert struct.unpack_from("<Q", raw, p + 24 * 51)[0] == g.state and p + 24 * 51 + 8 == len(raw)


# ------------------------------------------------------------------ the host entries ----
def test_cv_rng_colours_equal_the_big_int_restatement():
    from multiviewstitch_amd import processor as P
    g = R.Rng()
    got, st = P.cv_rng_colours(25)
    assert got.tolist() == [list(g.colour()) for _ in range(25)] and st == g.state
    more, st2 = P.cv_rng_colours(10, st)                              # a state carried over two calls
    assert more.tolist() == [list(g.colour()) for _ in range(10)] and st2 == g.state
    both, st3 = P.cv_rng_colours(35)
    assert np.array_equal(both, np.concatenate([got, more])) and st3 == st2
    g = R.Rng(0xFEDCBA9876543210)
    got, st = P.cv_rng_colours(7, 0xFEDCBA9876543210)
    assert got.tolist() == [list(g.colour()) for _ in range(7)] and st == g.state
    assert P.cv_rng_colours(0)[1] == R.RNG_DEFAULT


def test_the_entries_without_a_device(tmp_path):
    from multiviewstitch_amd import _lib as L, processor as P
    lib = L.lib()
    for name in ("mvs_draw_overlays", "mvs_draw_overlays_dev", "mvs_cv_rng_colours", "mvs_match_overlays", "mvs_match_overlays_dev",
                 "mvs_sift_overlays", "mvs_sift_overlays_dev", "mvs_processor_match_overlays", "mvs_processor_sift_overlays",
                 "mvs_test_match_overlays_timed"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert C.sizeof(L.CDrawPrim) == 24 and L.DRAW_PRIM_DTYPE.itemsize == 24
    assert [L.CDrawPrim.x1.offset, L.CDrawPrim.kind.offset, L.CDrawPrim.size.offset, L.CDrawPrim.c.offset] == [8, 16, 17, 18]
    x = np.zeros((2, 8, 9, 3), np.uint8)
    out = np.zeros_like(x)

    def draw(prims, n=2, w=9, h=8, off=None, imgs=x, o=out):
        flat = np.array(prims, dtype=L.DRAW_PRIM_DTYPE).reshape(-1)
        off = np.array([0, len(flat), len(flat)] if off is None else off, np.int64)
        a = (n, w, h, L.ptr(imgs), L.ptr(off), L.ptr(flat), L.ptr(o))
        return lib.mvs_draw_overlays(*a), lib.mvs_draw_overlays_dev(*a, None)

    ok = P.draw_prim(L.DRAW_SEGMENT, 0, 0, 8, 7, 2)
    bad = [P.draw_prim(L.DRAW_SEGMENT, 0, 0, 9, 7, 2), P.draw_prim(L.DRAW_SEGMENT, 0, 0, 8, 8, 2), P.draw_prim(L.DRAW_SEGMENT, -1, 0, 8, 7, 2),
           P.draw_prim(L.DRAW_SEGMENT, 0, 0, 8, 7, 0), P.draw_prim(3, 1, 1), P.draw_prim(L.DRAW_DISC, 2 ** 20 + 1, 0), P.draw_prim(L.DRAW_RING, 0, -2 ** 20 - 1)]
    for q in bad:
        assert draw([ok, q]) == (E_INVALID, E_INVALID), q
    assert b"canvas 0, primitive 1" in lib.mvs_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(w=0), dict(h=16385), dict(off=[1, 1, 1]), dict(off=[0, 1, 0]), dict(imgs=None), dict(o=None)):
        assert draw([ok], **kw) == (E_INVALID, E_INVALID), kw
    m = np.array([[1, 2, 3, 4]], np.int32)
    moff = np.array([0, 1, 1], np.int64)
    y = np.zeros((2, 16, 9, 3), np.uint8)

    def match(n1=1, n2=2, w=9, h=8, mm=m, a=x, b=x):
        args = (n1, n2, w, h, L.ptr(a), L.ptr(b), L.ptr(moff), L.ptr(mm), None, L.ptr(y))
        return (lib.mvs_match_overlays(*args), lib.mvs_match_overlays_dev(*args, None),
                lib.mvs_processor_match_overlays(os.fsencode(str(tmp_path / "Match")), 0, *args[:8], 0, None, None))

    for kw in (dict(h=8193), dict(n1=0), dict(w=16385), dict(a=None), dict(mm=None), dict(mm=np.array([[9, 2, 3, 4]], np.int32)),
               dict(mm=np.array([[1, 2, 3, 8]], np.int32)), dict(mm=np.array([[1, -1, 3, 4]], np.int32))):
        assert match(**kw) == (E_INVALID,) * 3, kw
    assert b"pair (0, 0), match 0" in lib.mvs_last_error()
    keys = np.zeros((3, 4), np.float32)
    koff = np.array([0, 3, 3], np.int64)

    def sift(n=2, w=9, h=8, ko=koff, kk=keys, v=x):
        args = (n, w, h, L.ptr(v), L.ptr(np.asarray(ko, np.int64)), L.ptr(kk), L.ptr(out))
        return lib.mvs_sift_overlays(*args), lib.mvs_sift_overlays_dev(*args, None)

    for kw in (dict(n=0), dict(w=0), dict(h=16385), dict(ko=[0, 3, 2]), dict(kk=None), dict(v=None)):
        assert sift(**kw) == (E_INVALID, E_INVALID), kw
    sd = os.fsencode(str(tmp_path / "seq"))
    fa = (L.ptr(x), L.ptr(koff), L.ptr(keys))
    assert lib.mvs_processor_sift_overlays(sd, b"Other", 1, 2, 9, 8, *fa, 0, None) == E_INVALID
    assert lib.mvs_processor_sift_overlays(sd, b"Sift", 0, 2, 9, 8, *fa, 0, None) == E_INVALID
    assert lib.mvs_processor_sift_overlays(sd, b"Sift", 1, 2, 9, 8, *fa, 4, None) == E_INVALID
    prm = P.jpeg_encode_params(quality=0)
    assert lib.mvs_processor_sift_overlays(sd, b"Sift1", 1, 2, 9, 8, *fa, 0, C.byref(prm)) == E_INVALID
    assert lib.mvs_processor_match_overlays(os.fsencode(str(tmp_path / "Match")), 0, 1, 2, 9, 8, L.ptr(x), L.ptr(x), L.ptr(moff), L.ptr(m), 0, None,
                                            C.byref(prm)) == E_INVALID
    assert lib.mvs_processor_match_overlays(None, 0, 1, 2, 9, 8, L.ptr(x), L.ptr(x), L.ptr(moff), L.ptr(m), 0, None, None) == E_INVALID
    assert not os.path.exists(tmp_path / "Match") and not os.path.exists(tmp_path / "seq")       # refused before anything is created
    with pytest.raises(L.MvsError) as e:
        P.MatchOverlays(x[:1], x, [[m, m[:0]]], rng_state=np.zeros(1, np.int64))
    assert e.value.code == E_INVALID
    if L.device_count() == 0:
        calls = (lambda: P.DrawOverlays(x, [[ok], []]), lambda: P.MatchOverlays(x[:1], x, [[m, m[:0]]]), lambda: P.SiftOverlays(x, [keys, keys[:0]]),
                 lambda: P.MatchOverlayFiles(tmp_path / "Match", 0, x[:1], x, [[m, m[:0]]]),
                 lambda: P.SiftOverlayFiles(tmp_path / "seq", "Sift", x[None], [keys, keys[:0]]))
        for call in calls:
            with pytest.raises(L.MvsError) as e:
                call()
            assert e.value.code == E_NO_DEVICE
        assert not os.path.exists(tmp_path / "Match") and not os.path.exists(tmp_path / "seq")
