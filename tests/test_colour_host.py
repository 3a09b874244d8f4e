"""Host side of mvs_colour_vertices (include/mvs.h): symbols, the layout and defaults of mvs_colour_params, the argument checks (they run
before a device is needed), the file entry's errors, the coloured OBJ round trip, the conditions the scenes of tests/colour_scenes.py must
meet for the GPU comparison to demand equal bytes on every vertex, the restatement tests/ref_colour.py on a ramp texture, and the shared
rules header (csrc/colour_rules.h) as a stand-alone program under the address and undefined-behaviour sanitizers — on its own cases and
on scenes O and Q, against the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P, scene as S
from tests import colour_scenes as SC, ref_colour as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE, E_IO = -1, -4, -10


def _cam(w=16, h=12):
    return S.Camera(20.0, 20.0, w / 2 - 0.5, h / 2 - 0.5, np.eye(3), np.zeros(3), w, h)


def _call(cams=None, off=None, n_seq=1, V=4, points=True, normals=True, cam_off=True, cam_ptr=True, imgs=True, colours=True, prm=True,
          chain=(False, False, False), fn="mvs_colour_vertices", **fields):
    cams = [_cam(), _cam()] if cams is None else cams
    off = np.asarray([0, len(cams)] if off is None else off, np.int32)
    arr = (L.CCamera * max(1, len(cams)))(*[L.CCamera.of(c) for c in cams])
    px = max(1, sum(min(c.w, 64) * min(c.h, 64) for c in cams if c.w > 0 and c.h > 0))
    pts, nrm, im = np.zeros((max(V, 1), 3)), np.zeros((max(V, 1), 3)), np.zeros(3 * px, np.uint8)
    col, s, Rm, t = np.zeros((max(V, 1), 3), np.uint8), np.ones(8), np.tile(np.eye(3), (8, 1, 1)), np.zeros((8, 3))
    p = P.colour_params(**fields)
    args = (L.ptr(pts) if points else None, L.ptr(nrm) if normals else None, V, n_seq, L.ptr(s) if chain[0] else None,
            L.ptr(Rm) if chain[1] else None, L.ptr(t) if chain[2] else None, L.ptr(off) if cam_off else None, arr if cam_ptr else None,
            L.ptr(im) if imgs else None, None, C.byref(p) if prm else None, L.ptr(col) if colours else None, None)
    return getattr(L.lib(), fn)(*args, *((None,) if fn.endswith("_dev") else ()))


def test_symbols_and_params_layout():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_colour_default_params", "mvs_colour_vertices", "mvs_colour_vertices_dev", "mvs_obj_write_coloured", "mvs_obj_read_colours",
                 "mvs_processor_colour_model"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T = L.CColourParams
    assert C.sizeof(T) == 24
    assert [getattr(T, k).offset for k, _ in T._fields_] == [0, 8, 16, 20, 23]
    assert [k for k, _ in T._fields_] == ["min_cos", "occ_tol", "flags", "fill", "reserved"]
    p = P.colour_params()
    assert (p.min_cos, p.occ_tol, p.flags, list(p.fill), p.reserved) == (0.2, 0.01, 0, [128, 128, 128], 0)
    ref = R.params()
    assert (ref["min_cos"], ref["occ_tol"], ref["flags"], tuple(ref["fill"])) == (p.min_cos, p.occ_tol, p.flags, tuple(p.fill))
    assert L.COLOUR_BEST == R.BEST == 1
    q = P.colour_params(fill=(1, 2, 3), flags=L.COLOUR_BEST, min_cos=0.5)
    assert (list(q.fill), q.flags, q.min_cos) == ([1, 2, 3], 1, 0.5)
    assert lib.mvs_abi_version() == 4
    with pytest.raises(L.MvsError):
        P.colour_params(levels=3)


BAD = [dict(points=False), dict(normals=False), dict(cam_off=False), dict(cam_ptr=False), dict(imgs=False), dict(colours=False),
       dict(V=-1), dict(V=2 ** 31 - 1), dict(n_seq=0), dict(off=[1, 2]), dict(off=[0, 2, 1], n_seq=2), dict(cams=[], off=[0, 0]),
       dict(cams=[_cam(w=1)]), dict(cams=[_cam(h=1)]), dict(cams=[_cam(w=0)]), dict(cams=[_cam(h=-3)]), dict(cams=[_cam(), _cam(w=18)]),
       dict(cams=[_cam(), _cam(h=10)]), dict(cams=[_cam(w=65536, h=32768)]), dict(cams=[_cam()] * 500),
       dict(chain=(True, False, False)), dict(chain=(True, True, False)), dict(chain=(False, True, True)),
       dict(min_cos=0.0), dict(min_cos=-0.2), dict(min_cos=1.0000001), dict(min_cos=math.nan), dict(min_cos=math.inf),
       dict(occ_tol=0.0), dict(occ_tol=-0.01), dict(occ_tol=math.nan), dict(occ_tol=math.inf), dict(flags=2), dict(flags=3), dict(flags=-1),
       dict(reserved=1), dict(reserved=255)]


def _id(kw):
    return ",".join(f"{k}={[(c.w, c.h) for c in v][:3] if k == 'cams' else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BAD, ids=[_id(kw) for kw in BAD])
def test_argument_errors_need_no_device(kw):
    assert _call(**kw) == E_INVALID
    assert b"mvs_colour_vertices:" in L.lib().mvs_last_error()
    assert _call(fn="mvs_colour_vertices_dev", **kw) == E_INVALID
    assert b"mvs_colour_vertices_dev:" in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    # the arrays of _call live on the host: with a device present the _dev form would hand them to a kernel, so it is called only where
    # the answer is MVS_E_NO_DEVICE (tests/test_gpu_colour.py holds the device form on device arrays)
    for fn in ("mvs_colour_vertices",) + (("mvs_colour_vertices_dev",) if L.device_count() == 0 else ()):
        assert _call(fn=fn) in (0, E_NO_DEVICE)
        assert _call(fn=fn, prm=False) in (0, E_NO_DEVICE)                                     # NULL params: the defaults
        assert _call(fn=fn, V=0) in (0, E_NO_DEVICE)
        assert _call(fn=fn, chain=(True, True, True), cams=[_cam(w=2, h=2)] * 3, off=[0, 1, 1, 3], n_seq=3) in (0, E_NO_DEVICE)
        assert _call(fn=fn, min_cos=1.0, occ_tol=1e-300, flags=1, cams=[_cam()] * 400) in (0, E_NO_DEVICE)


def test_python_entries_check_their_shapes():
    cams = [[_cam(), _cam()]]
    pts, nrm, imgs = np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((2, 12, 16, 3), np.uint8)
    for bad in (dict(points=np.zeros((4, 2))), dict(normals=np.zeros((3, 3))), dict(imgs=imgs[:1]), dict(depths=np.zeros((2, 12, 15), np.float32)),
                dict(scales=[1.0])):
        kw = dict(points=pts, normals=nrm, imgs=imgs)
        kw.update(bad)
        with pytest.raises(L.MvsError):
            P.ColourVertices(kw.pop("points"), kw.pop("normals"), cams, kw.pop("imgs"), **kw)


def test_the_file_entry_reports_its_errors_before_it_writes(tmp_path):
    cams = [[_cam(), _cam()]]
    d = tmp_path / "seq0"
    d.mkdir()
    model, srt, out = str(tmp_path / "m.obj"), str(tmp_path / "SRT.txt"), str(tmp_path / "out.obj")
    IO.WriteObj(model, np.array([[0, 0, 2.0], [0.1, 0, 2], [0, 0.1, 2]]), np.tile([0, 0, -1.0], (3, 1)), np.array([[0, 1, 2]], np.int32))
    IO.write_srt_txt(srt, [1.0], [np.eye(3)], [np.zeros(3)])
    with pytest.raises(L.MvsError) as e:
        P.ColourModelFiles(model, srt, [str(d)], cams, out, P.colour_params(min_cos=0.0))
    assert e.value.code == E_INVALID and "mvs_processor_colour_model" in str(e.value)
    with pytest.raises(L.MvsError) as e:
        P.ColourModelFiles(model, srt, [str(d)], [[_cam(), _cam(w=18)]], out)
    assert e.value.code == E_INVALID
    with pytest.raises(L.MvsError):
        P.ColourModelFiles(model, srt, [str(d), str(d)], cams, out)
    with pytest.raises(L.MvsError) as e:
        P.ColourModelFiles(model, srt, [str(d)], cams, out, znear=0.0)
    assert e.value.code == E_INVALID
    lib = L.lib()
    off, arr = L.seq_cams(cams)
    dirs = (C.c_char_p * 1)(os.fsencode(str(d)))
    args = lambda **kw: tuple({**dict(m=os.fsencode(model), s=os.fsencode(srt), n=1, o=L.ptr(off), c=arr, d=dirs, p=None, zn=0.01, zf=2000.0,
                                      out=os.fsencode(out), nc=None), **kw}.values())
    for kw in (dict(m=None), dict(s=None), dict(d=None), dict(out=None), dict(n=0), dict(o=None), dict(c=None)):
        assert lib.mvs_processor_colour_model(*args(**kw)) == E_INVALID
    if L.device_count() > 0:                                                                 # the files are opened once a device is there
        with pytest.raises(L.MvsError) as e:
            P.ColourModelFiles(str(tmp_path / "none.obj"), srt, [str(d)], cams, out)
        assert e.value.code == E_IO
        with pytest.raises(L.MvsError) as e:                                                 # no frames: reported with the path
            P.ColourModelFiles(model, srt, [str(d)], cams, out)
        assert e.value.code == E_IO and "00000.jpg" in str(e.value)
    else:
        assert lib.mvs_processor_colour_model(*args()) == E_NO_DEVICE
    assert not os.path.exists(out)


def test_coloured_obj_round_trip(tmp_path):
    """every byte value survives `v x y z r g b` with r = byte / 255 printed by %g, in both channel orders; mvs_obj_read reads the
    geometry of the coloured file as it reads the plain one; a line with fewer than six numbers is reported with its number"""
    V = 256
    rng = np.random.default_rng(3)
    pts, nrm = rng.normal(size=(V, 3)), rng.normal(size=(V, 3))
    fac = rng.integers(0, V, (50, 3)).astype(np.int32)
    col = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 7) % 256], axis=1).astype(np.uint8)
    plain, rgb, bgr = (str(tmp_path / n) for n in ("plain.obj", "rgb.obj", "bgr.obj"))
    IO.WriteObj(plain, pts, nrm, fac)
    IO.WriteObjColoured(rgb, pts, col, nrm, fac, "RGB")
    IO.WriteObjColoured(bgr, pts, col[:, ::-1], nrm, fac, "BGR")
    assert open(rgb, "rb").read().replace(b"rgb.obj", b"bgr.obj") == open(bgr, "rb").read()        # the file holds r g b either way
    assert np.array_equal(IO.ReadObjColours(rgb, "RGB"), col) and np.array_equal(IO.ReadObjColours(rgb, "BGR"), col[:, ::-1])
    for a, b in zip(IO.ReadObj(plain), IO.ReadObj(rgb)):
        assert np.array_equal(a, b)
    first_v = [ln for ln in open(rgb).read().splitlines() if ln.startswith("v ")][0].split()
    assert len(first_v) == 7 and first_v[4:] == ["0", "1", "0"]
    for with_n, with_f in ((False, True), (True, False), (False, False)):                            # `v` lines alone; no facets
        IO.WriteObjColoured(rgb, pts, col, nrm if with_n else None, fac if with_f else None)
        assert np.array_equal(IO.ReadObjColours(rgb), col)
        assert np.array_equal(IO.ReadObj(rgb)[0], IO.ReadObj(plain)[0])
    with pytest.raises(L.MvsError) as e:
        IO.ReadObjColours(plain)
    assert e.value.code == E_IO and "line" in str(e.value) and "fewer than six" in str(e.value)
    with pytest.raises(L.MvsError):
        IO.WriteObjColoured(rgb, pts, col[:10])
    with pytest.raises(L.MvsError):
        IO.WriteObjColoured(rgb, pts, col, order="GBR")
    lib = L.lib()
    buf = np.zeros((V, 3), np.uint8)
    IO.WriteObjColoured(rgb, pts, col)
    assert lib.mvs_obj_read_colours(os.fsencode(rgb), V - 1, L.ptr(buf), L.JPEG_RGB) == E_INVALID
    assert lib.mvs_obj_read_colours(os.fsencode(rgb), V, L.ptr(buf), 2) == E_INVALID
    assert lib.mvs_obj_read_colours(os.fsencode(rgb), V, None, L.JPEG_RGB) == E_INVALID
    assert lib.mvs_obj_write_coloured(os.fsencode(rgb), V, L.ptr(pts), None, None, L.JPEG_RGB, 0, None) == E_INVALID
    assert lib.mvs_obj_read_colours(os.fsencode(str(tmp_path / "none.obj")), V, L.ptr(buf), L.JPEG_RGB) == E_IO


# ------------------------------------------------------------------ the scenes and the restatement ----
@pytest.mark.parametrize("name", SC.NAMES)
def test_scene_conditions(name):
    """every decision an fp64 operation feeds clears MARGIN, so that a last-bit difference cannot move it and the GPU comparison may
    demand equal bytes with no vertex set aside.  A range test met with equality is exact by construction (scene E: powers of two) or
    absent; a tie of MVS_COLOUR_BEST is a tie of integers.  And the scenes hold what they are there for"""
    sc = SC.scene(name)
    assert len(sc["points"]) <= 3000 and sc["imgs"].shape[0] <= 17 and sc["imgs"].shape[1:] == (32, 40, 3)
    refs = [SC.reference(name, f) for f in (0, R.BEST)] + ([SC.reference(name, 0, False)] if sc["depths"] is not None else [])
    for ref in refs:
        for kind, m in ref["margins"].items():
            assert m >= SC.MARGIN, (kind, m)
        assert ref["exact_range"] == (2 if name == "E" else 0)
    blend, best = refs[0], refs[1]
    assert np.array_equal(blend["n_views"], best["n_views"]) and np.array_equal(blend["accepted"], best["accepted"])
    one = blend["n_views"] == 1
    assert np.array_equal(blend["colours"][one], best["colours"][one])
    if name == "P":
        assert (blend["n_views"] >= 2).sum() * 2 >= len(sc["points"])
    if name in ("O", "Q"):
        rj = blend["rejected"]
        assert rj["behind"] > 30 and rj["outside"] > 30 and rj["facing"] > 30 and rj["occluded"] > 30
        back = np.arange(len(sc["points"]) // 2, len(sc["points"]))
        assert (blend["colours"][back] != refs[2]["colours"][back]).any(axis=1).sum() > 100
        front_views = [0, 1] if name == "O" else [0, 2]
        hidden, bare = blend["accepted"][back][:, front_views].sum(), refs[2]["accepted"][back][:, front_views].sum()
        assert bare > 400 and hidden * 4 < bare                                                      # C4 alone hides the back sheet from the front
    if name == "E":
        n = blend["n_views"]
        assert blend["accepted"][[0, 3, 4, 5, 6], 0].sum() == 0                                      # camera 0 takes none of them
        assert blend["accepted"][1, 0] and blend["accepted"][2, 0] and (n[[4, 5, 6]] == 0).all()
        x1, x2 = blend["xy"][1, 0, 0], blend["xy"][2, 0, 0]
        assert x1 == 39.0 and x2 == 0.0 and blend["xy"][3, 0, 0] == -1.0 / 64
        assert (blend["colours"][[4, 5, 6]] == 128).all()
        assert blend["wq"][7, 1] == blend["wq"][7, 2] > 0 and not blend["accepted"][7, 0] and blend["best_ties"] >= 1
        assert not np.array_equal(best["colours"][7], blend["colours"][7])                           # the tie goes to view 1, the blend mixes both
    if name.startswith("S"):
        assert (blend["n_views"] > 0).all()


def test_scene_e_edges_sample_single_pixels():
    """camera 0 alone: the vertex on x = w - 1 gets the mean of pixels (39, 19) and (39, 20) — y = 19.5 —, the one on x = 0 likewise"""
    sc = SC.scene("E")
    ref = R.colour(sc["points"], sc["normals"], [sc["cameras"][0][:1]], sc["imgs"][:1])
    img = sc["imgs"][0].astype(np.int64)
    assert np.array_equal(ref["colours"][1], (img[19, 39] + img[20, 39] + 1) // 2)                   # y = 16 * 0.25 + 15.5 = 19.5
    assert np.array_equal(ref["colours"][2], (img[11, 0] + img[12, 0] + 1) // 2)                     # y = 11.5
    assert list(ref["n_views"]) == [0, 1, 1, 0, 0, 0, 0, 0, 1]


def test_ramp_texture():
    """on the ramp of scene P_RAMP (3 levels per column, 1 per row) every coloured vertex is within 1 level of the ramp's value at its
    projection: the bilinear sample of a linear function is exact up to the 1 / 512 pixel the fractions are rounded by (4 levels per
    pixel x 2 / 512), plus the half level of C8.  One camera at a time, blend and BEST; the restatement alone is tested here"""
    sc = SC.scene("P_RAMP")
    seen = 0
    for i, cam in enumerate(sc["cameras"][0]):
        for flags in (0, R.BEST):
            ref = R.colour(sc["points"], sc["normals"], [[cam]], sc["imgs"][i:i + 1], sc["depths"][i:i + 1], p=R.params(flags=flags))
            ok = ref["n_views"] == 1
            for ch in range(3):
                want = SC.ramp_value(ref["xy"][ok, 0, 0], ref["xy"][ok, 0, 1], ch)
                assert np.abs(ref["colours"][ok, ch].astype(np.float64) - want).max() <= 1.0
            seen += int(ok.sum())
    assert seen > 3000
    # all three cameras: the blend stays between the lowest and the highest single view, within the same level
    ref = SC.reference("P_RAMP")
    ok = ref["n_views"] > 0
    vals = np.stack([SC.ramp_value(ref["xy"][:, v, 0], ref["xy"][:, v, 1], 0) for v in range(3)], axis=1)
    vals_lo = np.where(ref["accepted"], vals, np.inf).min(axis=1)
    vals_hi = np.where(ref["accepted"], vals, -np.inf).max(axis=1)
    c = ref["colours"][:, 0].astype(np.float64)
    assert (c[ok] >= vals_lo[ok] - 1.0).all() and (c[ok] <= vals_hi[ok] + 1.0).all()


# ------------------------------------------------------------------ the shared rules ----
def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "colour_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "colour_rules.cpp"), "-o", exe])
    return exe


def write_scene(path, sc, p, with_depths=True):
    """the input of tests/colour_rules.cpp"""
    views = [(k, c) for k, seq in enumerate(sc["cameras"]) for c in seq]
    N, V = len(views), len(sc["points"])
    has_d = with_depths and sc["depths"] is not None
    with open(path, "wb") as fh:
        fh.write(np.asarray([V, N, len(sc["cameras"]), SC.W, SC.H, p["flags"], int(has_d), int(sc["scales"] is not None)], np.int32).tobytes())
        fh.write(np.asarray([p["min_cos"], p["occ_tol"]], np.float64).tobytes())
        fh.write(np.asarray(list(p["fill"]) + [0], np.uint8).tobytes())
        for k, c in views:
            fh.write(np.concatenate([[c.fx, c.fy, c.cx, c.cy], np.asarray(c.R, np.float64).reshape(9), np.asarray(c.t, np.float64).reshape(3), [k]]).tobytes())
        if sc["scales"] is not None:
            for k in range(len(sc["cameras"])):
                fh.write(np.concatenate([[sc["scales"][k]], np.asarray(sc["Rs"][k], np.float64).reshape(9), np.asarray(sc["ts"][k], np.float64).reshape(3)]).tobytes())
        fh.write(np.ascontiguousarray(sc["points"], np.float64).tobytes())
        fh.write(np.ascontiguousarray(sc["normals"], np.float64).tobytes())
        fh.write(np.ascontiguousarray(sc["imgs"], np.uint8).tobytes())
        if has_d:
            fh.write(np.ascontiguousarray(sc["depths"], np.float32).tobytes())


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """tests/colour_rules.cpp: a 2 x 2 image whose corners are the corners of the one bilinear cell, a hair outside, behind, NaN, facing
    away, C4 at both sides of occ_tol and on an empty pixel, equal weights, the tie of BEST, the key order, the smallest weight and the
    map of C1, on heap blocks of exact size; then C1-C8 of the header on scenes O, Q and E against the restatement, byte for byte (host
    code, no contraction)"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "colour rules ok" in run.stdout, run.stdout + run.stderr
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for name, flags, with_depths in (("O", 0, True), ("O", R.BEST, True), ("O", 0, False), ("Q", 0, True), ("Q", R.BEST, True), ("E", R.BEST, True)):
        sc, ref = SC.scene(name), SC.reference(name, flags, with_depths)
        write_scene(fin, sc, R.params(flags=flags), with_depths)
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = open(fout, "rb").read()
        V = len(sc["points"])
        assert len(raw) == 7 * V
        assert np.array_equal(np.frombuffer(raw[:3 * V], np.uint8).reshape(V, 3), ref["colours"]), (name, flags, with_depths)
        assert np.array_equal(np.frombuffer(raw[3 * V:], np.int32), ref["n_views"])
