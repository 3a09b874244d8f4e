"""Host side of mvs_refine_depth_maps (include/mvs.h): symbols, the layout of mvs_depth_refine_params, the argument checks (they run
before a device is needed), the file entry's I/O errors, properties of the numpy restatement tests/ref_depth_refine.py, the conditions the
scenes of tests/depth_refine_scenes.py must meet for the GPU comparison to be exact, what the refinement achieves on scenes A and B, and the
shared rules header (csrc/depth_refine_rules.h) as a stand-alone program under the address and undefined-behaviour sanitizers — on its own
cases and on scene B, against the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P, scene as S
from tests import depth_refine_scenes as SC, ref_depth_refine as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE, E_IO = -1, -4, -10


def _cam(w=16, h=12, fx=20.0, fy=20.0):
    return S.Camera(fx, fy, w / 2 - 0.5, h / 2 - 0.5, np.eye(3), np.zeros(3), w, h)


def _call(cams=None, off=None, n_seq=1, cam_off=True, cam_ptr=True, imgs=True, depths=True, prm=True, out=True, alias=False, fn="mvs_refine_depth_maps",
          **fields):
    cams = [_cam(), _cam()] if cams is None else cams
    off = np.asarray([0, len(cams)] if off is None else off, np.int32)
    arr = (L.CCamera * max(1, len(cams)))(*[L.CCamera.of(c) for c in cams])
    px = max(1, sum(min(c.w, 64) * min(c.h, 64) for c in cams if c.w > 0 and c.h > 0))
    d, o, im = np.zeros(px, np.float32), np.zeros(px, np.float32), np.zeros(3 * px, np.uint8)
    p = P.depth_refine_params(**fields)
    args = (n_seq, L.ptr(off) if cam_off else None, arr if cam_ptr else None, L.ptr(im) if imgs else None, L.ptr(d) if depths else None,
            C.byref(p) if prm else None, (L.ptr(d) if alias else L.ptr(o)) if out else None, None, None, None)
    return getattr(L.lib(), fn)(*args, *((None,) if fn.endswith("_dev") else ()))


def test_symbols_and_params_layout():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_depth_refine_default_params", "mvs_refine_depth_maps", "mvs_refine_depth_maps_dev", "mvs_processor_refine_depths"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T = L.CDepthRefineParams
    assert C.sizeof(T) == 48 and T.rel_range.offset == 16 and T.ssd_err.offset == 24 and T.ssd_win.offset == 32 and T.flags.offset == 44
    p = P.depth_refine_params()
    assert (p.dsp_min, p.dsp_max, p.rel_range, p.ssd_err) == (0.0025, 0.3, 0.04, 40.0)
    assert (p.ssd_win, p.ref_frm_count, p.steps, p.flags) == (7, 5, 8, L.REFINE_SUBSTEP) and L.REFINE_SUBSTEP == R.SUBSTEP == 1
    assert lib.mvs_abi_version() == 4
    with pytest.raises(L.MvsError):
        P.depth_refine_params(window=3)


BAD = [dict(cam_off=False), dict(cam_ptr=False), dict(imgs=False), dict(depths=False), dict(prm=False), dict(out=False), dict(alias=True),
       dict(n_seq=0), dict(off=[1, 2]), dict(off=[0, 2, 1], n_seq=2), dict(cams=[_cam(w=0)]), dict(cams=[_cam(h=-3)]), dict(cams=[_cam(fx=0.0)]),
       dict(cams=[_cam(fy=0.0)]), dict(cams=[_cam(), _cam(w=18)]), dict(cams=[_cam(), _cam(h=10)]), dict(cams=[_cam(w=65536, h=32768)]),
       dict(dsp_min=math.nan), dict(dsp_max=math.inf), dict(rel_range=math.nan), dict(ssd_err=math.inf), dict(ssd_err=math.nan),
       dict(dsp_min=0.0), dict(dsp_min=-0.1), dict(dsp_min=0.4), dict(rel_range=0.0), dict(rel_range=-0.04), dict(rel_range=1.0), dict(ssd_err=-1e-9),
       dict(ssd_win=-1), dict(ssd_win=16), dict(ref_frm_count=0), dict(ref_frm_count=-1), dict(ref_frm_count=4), dict(ref_frm_count=11),
       dict(ref_frm_count=10), dict(steps=0), dict(steps=64), dict(flags=2), dict(flags=3), dict(flags=-1)]


def _id(kw):
    return ",".join(f"{k}={[(c.w, c.h, c.fx, c.fy) for c in v] if k == 'cams' else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BAD, ids=[_id(kw) for kw in BAD])
def test_argument_errors_need_no_device(kw):
    assert _call(**kw) == E_INVALID
    assert b"mvs_refine_depth_maps:" in L.lib().mvs_last_error()
    assert _call(fn="mvs_refine_depth_maps_dev", **kw) == E_INVALID
    assert b"mvs_refine_depth_maps_dev:" in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    assert _call() in (0, E_NO_DEVICE)
    assert _call(cams=[_cam(), _cam(w=18), _cam(w=18)], off=[0, 1, 1, 3], n_seq=3) in (0, E_NO_DEVICE)      # sizes differ between sequences; one is empty
    assert _call(ssd_win=15, ref_frm_count=9, steps=63, ssd_err=0.0, dsp_min=0.3, rel_range=0.999, flags=0) in (0, E_NO_DEVICE)
    assert _call(ssd_win=0, ref_frm_count=1, steps=1) in (0, E_NO_DEVICE)


def test_the_file_entry_reports_its_io_errors_before_it_writes(tmp_path):
    cams = [[_cam(), _cam()]]
    imgs = [np.zeros((2, 12, 16, 3), np.uint8)]
    d = tmp_path / "seq0"
    os.makedirs(d / "DATA" / "Render")
    IO.SaveDepth(str(d / "DATA" / "Render" / "_depth0.raw"), np.zeros((12, 16)))
    with pytest.raises(L.MvsError) as e:
        P.RefineDepthFiles([str(d)], cams, imgs)
    assert e.value.code == E_IO and "_depth1.raw" in str(e.value) and not (d / "DATA" / "Refine").exists()
    (d / "DATA" / "Render" / "_depth1.raw").write_bytes(b"\0" * (4 * 12 * 16 - 4))       # one float short
    with pytest.raises(L.MvsError) as e:
        P.RefineDepthFiles([str(d)], cams, imgs)
    assert e.value.code == E_IO and "_depth1.raw" in str(e.value) and not (d / "DATA" / "Refine").exists()
    IO.SaveDepth(str(d / "DATA" / "Render" / "_depth1.raw"), np.zeros((12, 16)))        # both rasters there: the parameters are checked next
    with pytest.raises(L.MvsError) as e:
        P.RefineDepthFiles([str(d)], cams, imgs, P.depth_refine_params(steps=0))
    assert e.value.code == E_INVALID and "mvs_processor_refine_depths" in str(e.value) and not (d / "DATA" / "Refine").exists()
    with pytest.raises(L.MvsError):
        P.RefineDepthFiles([str(d)], cams, [imgs[0][:, :, :8]])                          # an image stack of the wrong size never reaches the library
    lib = L.lib()
    off, arr = L.seq_cams(cams)
    dirs = (C.c_char_p * 1)(os.fsencode(str(d)))
    assert lib.mvs_processor_refine_depths(1, dirs, L.ptr(off), arr, None, None) == E_INVALID
    assert lib.mvs_processor_refine_depths(1, None, L.ptr(off), arr, L.ptr(imgs[0]), None) == E_INVALID
    assert lib.mvs_processor_refine_depths(0, dirs, L.ptr(off), arr, L.ptr(imgs[0]), None) == E_INVALID


# ------------------------------------------------------------------ the restatement ----
def test_grey_and_references():
    assert R.grey(np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [90, 140, 35]], np.uint8)).tolist() == \
        [0, 255, 76, 150, 29, (4899 * 90 + 9617 * 140 + 1868 * 35 + 8192) >> 14]
    assert R.references(0, 6, 5) == [1, 2] and R.references(2, 6, 5) == [0, 1, 3, 4] and R.references(5, 6, 5) == [3, 4]
    assert R.references(3, 6, 1) == [] and R.references(3, 6, 3) == [2, 4] and R.references(1, 6, 9) == [0, 2, 3, 4, 5] and R.references(0, 1, 5) == []


@pytest.mark.parametrize("name", SC.NAMES)
def test_pass_through_is_bit_exact(name):
    """every pixel without an accepted hypothesis holds its input bits — the planted NaNs (with their payloads), infinities, negative
    values, -0.0, zeros and the values just outside the range among them; a candidate reports sum >= 0 exactly when it had an eligible k"""
    _, _, depths, p = SC.scene(name)
    for flags in (0, R.SUBSTEP):
        for dsp, ref in zip(depths, SC.reference(name, flags)):
            keep = ref["k"] == R.NONE
            assert np.array_equal(ref["out"].view(np.uint32)[keep], dsp.view(np.uint32)[keep])
            assert ((ref["sum"] == -1) == (ref["cnt"] == 0)).all() and (ref["cnt"][~keep] > 0).all() and (np.abs(ref["k"][~keep]) <= p["steps"]).all()
            for f, fr in enumerate(ref["frames"]):
                assert (ref["cnt"][f][~fr["cand"]] == 0).all() and (ref["k"][f][~fr["cand"]] == R.NONE).all()
    if name.startswith("E"):
        (dsp,), (ref,) = depths, SC.reference(name)
        for f in range(len(dsp)):
            row = ref["out"][f, 8 + 2 * f, 6:6 + len(SC.PLANTS)]
            assert row[:8].view(np.uint32).tolist() == np.asarray(SC.PLANTS[:8], np.float32).view(np.uint32).tolist()
            assert (ref["cnt"][f, 8 + 2 * f, 6:6 + 8] == 0).all()
        assert ref["out"][2, 5, 10:12].view(np.uint32).tolist() == [0x7fc12345, 0xffc00001]
        assert np.signbit(ref["out"][0, 8, 6 + 4]) and ref["out"][0, 8, 6 + 4] == 0            # -0.0 keeps its sign


def test_one_frame_and_one_reference_window_return_the_input():
    for name in ("D", "E_R1"):
        _, _, depths, _ = SC.scene(name)
        for dsp, ref in zip(depths, SC.reference(name)):
            assert ref["out"].tobytes() == dsp.tobytes() and (ref["k"] == R.NONE).all() and (ref["sum"] == -1).all() and (ref["cnt"] == 0).all()


def test_one_colour_images_give_k_zero_and_the_input_bytes():
    cameras, imgs, depths, p = SC.scene("A")
    flat = [np.full_like(i, 77) for i in imgs]
    for flags in (0, R.SUBSTEP):
        (ref,) = R.refine(cameras, flat, depths, dict(p, flags=flags))
        zero, other = SC.one_colour_expectation(ref, depths[0], p["steps"])
        print("k* = 0:", zero, "pixels; another k*:", other)
        assert zero > 1000 and other < 0.02 * zero
    # scene E under ref_frm_count = 3: frame 0's only reference is frame 1, and both are of one colour
    (ref,), (dsp,) = SC.reference("E_R3"), SC.scene("E_R3")[2]
    k0 = ref["k"][0]
    assert (ref["sum"][0][ref["cnt"][0] > 0] == 0).all() and (k0 == 0).sum() > 10 * ((k0 != 0) & (k0 != R.NONE)).sum() > 0
    assert (ref["out"][0].view(np.uint32) == dsp[0].view(np.uint32))[(k0 == 0) | (k0 == R.NONE)].all()


def test_the_tie_order_of_rule_6_on_a_constructed_pixel():
    K = 3
    sums = np.array([[12, 30, 6, 6, 12, 3, 9]], np.int64).T              # k = -3 .. 3
    cnts = np.array([[2, 1, 1, 1, 2, 0, 3]], np.int64).T
    # ratios 6, 30, 6, 6, 6, -, 3 -> k = 3 wins outright
    assert R.choose(sums, cnts, K)[0].tolist() == [3]
    cnts[6] = 0                                                          # without it: 6 at k = -3, -1, 0, 1 -> the smallest |k|
    assert R.choose(sums, cnts, K)[0].tolist() == [0]
    cnts[3] = 0                                                          # -1 and 1 tie: k < 0 wins
    assert R.choose(sums, cnts, K)[0].tolist() == [-1]
    cnts[2] = 0                                                          # -3 (12 / 2) and 1 (12 / 2): the smaller |k|
    assert R.choose(sums, cnts, K)[0].tolist() == [1]
    cnts[:] = 0
    best, any_k = R.choose(sums, cnts, K)
    assert best.tolist() == [R.NONE] and not any_k.any()
    big = np.array([[490000000, 499999999]], np.int64).T                 # products beyond 2^31
    assert R.choose(np.concatenate([big, big[:1]]), np.array([[8, 7, 0]], np.int64).T, 1)[0].tolist() == [-1]


@pytest.mark.parametrize("name", ("A", "B", "C", "E", "E_N0", "E_R9"))
def test_the_substep_stays_inside_half_a_step(name):
    _, _, depths, p = SC.scene(name)
    step = p["rel_range"] / p["steps"]
    moved = 0
    for dsp, on, off in zip(depths, SC.reference(name, R.SUBSTEP), SC.reference(name, 0)):
        assert np.array_equal(on["k"], off["k"]) and np.array_equal(on["sum"], off["sum"]) and np.array_equal(on["cnt"], off["cnt"])
        for f, fr in enumerate(on["frames"]):
            o = fr["offset"]
            # rule 8 never leaves [k* - 0.5, k* + 0.5]: c0 is the smallest of the three, so |c- - c+| <= (c- - c0) + (c+ - c0) = den; an
            # end of the interval is reached only when a neighbour's mean equals the winner's (the winner then won by rule 6's tie order)
            # In fp64 the bound holds to 1e-6: the means are quotients of integers, sums below 5e8 over counts of at most 8, so two
            # different means lie at least 1 / 56 apart, and the rounding of c- - 2 c0 (half an ulp of a value below 6.3e7) moves a den
            # of 1 / 56 by less than 2^-53 * 6.3e7 * 56 < 4e-7 of itself.
            assert (np.abs(o) <= 0.5 + 1e-6).all(), float(np.abs(o).max())
            K, idx = p["steps"], np.arange(len(o))
            edge = np.abs(o) >= 0.5
            bi = np.where(edge, fr["best"], 0) + K
            lo, hi = np.clip(bi - 1, 0, 2 * K), np.clip(bi + 1, 0, 2 * K)
            s, c = fr["sums"], fr["cnts"]
            tie = (s[lo, idx] * c[bi, idx] == s[bi, idx] * c[lo, idx]) | (s[hi, idx] * c[bi, idx] == s[bi, idx] * c[hi, idx])
            assert tie[edge].all()
            acc = on["k"][f] != R.NONE
            d0 = dsp[f][acc].astype(np.float64)
            rel = on["out"][f][acc].astype(np.float64) / d0 - 1.0
            k = on["k"][f][acc].astype(np.float64)
            assert (rel > (k - 0.5) * step - 1e-6).all() and (rel < (k + 0.5) * step + 1e-6).all()      # 1e-6: the float32 of out
            moved += int((on["out"][f] != off["out"][f]).sum())
    assert moved > (0 if name == "E_R9" else 100)


@pytest.mark.parametrize("name", SC.NAMES)
def test_scene_conditions(name):
    """every decision an fp64 operation feeds clears its margin, so that a last-bit difference cannot move it; and the scenes hold what
    they are there for"""
    cameras, imgs, depths, p = SC.scene(name)
    for k, ref in enumerate(SC.reference(name)):
        mg = ref["margins"]
        print(name, k, {kind: f"{v:.2e}" for kind, v in mg.items()})
        n = len(cameras[k])
        if n > 1 and p["ref_frm_count"] > 1:
            assert set(mg) >= {"coord", "z", "bound", "accept"}
        assert mg.get("coord", 1.0) >= SC.MARGIN and mg.get("z", 1.0) > SC.MARGIN and mg.get("accept", 1.0) >= SC.MARGIN
        assert mg.get("bound", 1.0) >= SC.BOUND_MARGIN
        seen = {key: sum(fr["seen"][key] for fr in ref["frames"]) for key in ("dead", "behind", "outside")}
        accepted = int((ref["k"] != R.NONE).sum())
        rejected = int(((ref["k"] == R.NONE) & (ref["cnt"] > 0)).sum())
        no_k = int(sum((fr["cand"] & (ref["cnt"][f] == 0)).sum() for f, fr in enumerate(ref["frames"])))
        print(name, k, seen, "accepted", accepted, "rejected", rejected, "candidates without an eligible k", no_k)
        if name in ("A", "B", "C", "AC", "E"):
            assert accepted > 300 and rejected > 30 and seen["dead"] > 100 and seen["outside"] > 50
        if name == "B":
            assert seen["behind"] > 1000 and no_k > 0
            assert len({int(c) for c in np.unique(ref["cnt"])}) >= 4                                      # 0, 1, 2 and 3 references took part
        if name == "A":
            w, h = cameras[k][0].w, cameras[k][0].h
            assert w % 16 and h % 16 and w > 32 and h > 16                                                 # several tiles, none of them whole


@pytest.mark.parametrize("name", ("A", "B"))
def test_refinement_recovers_the_planted_offsets(name):
    """measured on the restatement alone; tests/depth_refine_scenes.py records the run.  A later edit cannot pass on a scene where the
    refinement does nothing: the share may fall one tenth below the recorded one, the error after may rise one tenth above."""
    q, want = SC.quality(name), SC.QUALITY[name]
    print(name, q, "recorded", want)
    assert q["share"] >= 0.9 * want["share"] and want["share"] > 0.8
    assert abs(q["rms_before"] - want["rms_before"]) <= 0.1 * want["rms_before"]
    assert q["rms_after"] <= 1.1 * want["rms_after"] and q["rms_after"] < 0.25 * q["rms_before"]
    assert q["accepted"] > 1000


# ------------------------------------------------------------------ the shared rules ----
def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "depth_refine_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "depth_refine_rules.cpp"), "-o", exe])
    return exe


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """tests/depth_refine_rules.cpp: the tie order, border pixels, a window of one pixel in the corners, projections that land one past
    the interior, non-finite and out-of-range disparities on heap blocks of exact size; then rules 1-8 of the header on scene B (40 x 32,
    a camera behind the scene) against the restatement, with and without the substep: k, sum and cnt exactly, out bit for bit (host code,
    no contraction)"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "depth refine rules ok" in run.stdout, run.stdout + run.stderr
    (cams,), (imgs,), (dsp,), p = SC.scene("B")
    n, h, w = dsp.shape
    for flags in (0, R.SUBSTEP):
        (ref,) = SC.reference("B", flags)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as fh:
            fh.write(np.asarray([n, w, h, p["ssd_win"], p["ref_frm_count"], p["steps"], flags], np.int32).tobytes())
            fh.write(np.asarray([p["dsp_min"], p["dsp_max"], p["rel_range"], p["ssd_err"]], np.float64).tobytes())
            for c in cams:
                fh.write(np.concatenate([[c.fx, c.fy, c.cx, c.cy], np.asarray(c.R, np.float64).reshape(9), np.asarray(c.t, np.float64).reshape(3)]).tobytes())
            fh.write(imgs.tobytes())
            fh.write(dsp.tobytes())
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = open(fout, "rb").read()
        m = n * h * w
        assert len(raw) == 10 * m
        out = np.frombuffer(raw[:4 * m], np.uint32).reshape(n, h, w)
        sm = np.frombuffer(raw[4 * m:8 * m], np.int32).reshape(n, h, w)
        kk = np.frombuffer(raw[8 * m:9 * m], np.int8).reshape(n, h, w)
        cnt = np.frombuffer(raw[9 * m:], np.uint8).reshape(n, h, w)
        assert np.array_equal(kk, ref["k"]) and np.array_equal(sm, ref["sum"]) and np.array_equal(cnt, ref["cnt"])
        assert np.array_equal(out, ref["out"].view(np.uint32))
