"""Host side of mvs_grid_mincut and mvs_grabcut_masks (include/mvs.h): symbols, the layout of mvs_grabcut_params, the argument checks (they
run before a device is needed), properties of the restatement tests/ref_grabcut.py, the conditions the scenes of tests/grabcut_scenes.py
must meet for the GPU comparison to be exact, and the shared rules header (csrc/grabcut_rules.h) as a stand-alone program under the
address and undefined-behaviour sanitizers, against the restatement on scene data."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import grabcut_scenes as SC, ref_grabcut as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -4


def test_symbols_and_params_layout():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_grid_mincut", "mvs_grid_mincut_dev", "mvs_grabcut_default_params", "mvs_grabcut_masks", "mvs_grabcut_masks_dev",
                 "mvs_test_grabcut_trace"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T = L.CGrabCutParams
    assert C.sizeof(T) == 56 and T.hr.offset == 8 and T.vr.offset == 24 and T.gamma.offset == 32 and T.iters.offset == 40
    assert T.max_rounds.offset == 44 and T.reserved.offset == 48
    p = P.grabcut_params()
    assert (p.hl, p.hr, p.vl, p.vr, p.gamma, p.iters, p.max_rounds, p.reserved) == (0.1, 0.1, 0.1, 0.1, 50.0, 3, 4096, 0)
    assert lib.mvs_abi_version() == 4
    with pytest.raises(L.MvsError):
        P.grabcut_params(beta=1.0)


# ---------------------------------------------------------------- argument checks ----
def _mincut(n=1, gw=4, gh=3, excess=True, cap=True, side=True, max_rounds=8, dev=False, e_val=5, c_val=2):
    e = np.full((max(n, 1), 3, 4), e_val, np.int32)
    c = np.full((max(n, 1), 8, 3, 4), c_val, np.int32)
    s = np.zeros((max(n, 1), 3, 4), np.uint8)
    args = (n, gw, gh, L.ptr(e) if excess else None, L.ptr(c) if cap else None, max_rounds, L.ptr(s) if side else None, None)
    return L.lib().mvs_grid_mincut_dev(*args, None) if dev else L.lib().mvs_grid_mincut(*args)


BAD_CUT = [dict(excess=False), dict(cap=False), dict(side=False), dict(n=0), dict(gw=0), dict(gh=-1), dict(max_rounds=0), dict(gw=2 ** 14, gh=2 ** 13),
           dict(n=2 ** 10, gw=2 ** 11, gh=2 ** 11)]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kw", BAD_CUT, ids=[str(k) for k in BAD_CUT])
def test_mincut_argument_errors_need_no_device(kw, dev):
    assert _mincut(dev=dev, **kw) == E_INVALID
    assert (b"mvs_grid_mincut_dev" if dev else b"mvs_grid_mincut:") in L.lib().mvs_last_error()


def test_mincut_host_form_checks_capacities_and_headroom_before_a_device():
    assert _mincut(c_val=-1) == E_INVALID and b"negative" in L.lib().mvs_last_error()
    assert _mincut(e_val=2 ** 31 - 1 - 8 * 2, c_val=2) in (0, E_NO_DEVICE)                   # E + 8 C = 2^31 - 1: the last one allowed
    assert _mincut(e_val=2 ** 31 - 8 * 2, c_val=2) == E_INVALID and b"int32" in L.lib().mvs_last_error()
    assert _mincut(e_val=-2 ** 31, c_val=0) == E_INVALID
    # an entry that points outside the grid is ignored, a negative one included
    e, s = np.zeros((1, 1, 2), np.int32), np.zeros((1, 1, 2), np.uint8)
    c = np.full((1, 8, 1, 2), -7, np.int32)
    c[0, 4, 0, 0] = c[0, 0, 0, 1] = 3
    assert L.lib().mvs_grid_mincut(1, 2, 1, L.ptr(e), L.ptr(c), 4, L.ptr(s), None) in (0, E_NO_DEVICE)
    assert _mincut() in (0, E_NO_DEVICE)


def _grabcut(n=1, w=16, h=12, imgs=True, prm=True, mask=True, dev=False, trace=False, **fields):
    img = np.zeros((max(n, 1), 12, 16, 3), np.uint8)
    m = np.zeros((max(n, 1), 12, 16), np.uint8)
    p = P.grabcut_params(**fields)
    args = (n, w, h, L.ptr(img) if imgs else None, C.byref(p) if prm else None, L.ptr(m) if mask else None)
    if trace:
        return L.lib().mvs_test_grabcut_trace(*args, *([None] * 7))
    return L.lib().mvs_grabcut_masks_dev(*args, None, None) if dev else L.lib().mvs_grabcut_masks(*args, None)


BAD_GC = [dict(imgs=False), dict(prm=False), dict(mask=False), dict(n=0), dict(w=1), dict(h=1), dict(w=2 ** 14, h=2 ** 13),
          dict(n=2 ** 10, w=2 ** 11, h=2 ** 11), dict(hl=math.nan), dict(hr=-0.1), dict(vl=1.5), dict(vr=math.inf), dict(hl=0.5, hr=0.5),
          dict(vl=0.6, vr=0.6), dict(hl=1.0), dict(iters=0), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=math.nan), dict(gamma=1e6),
          dict(max_rounds=0)]


@pytest.mark.parametrize("kw", BAD_GC, ids=[str(k) for k in BAD_GC])
def test_grabcut_argument_errors_need_no_device(kw):
    assert _grabcut(**kw) == E_INVALID and b"mvs_grabcut_masks:" in L.lib().mvs_last_error()
    assert _grabcut(dev=True, **kw) == E_INVALID and b"mvs_grabcut_masks_dev" in L.lib().mvs_last_error()
    assert _grabcut(trace=True, **kw) == E_INVALID and b"mvs_test_grabcut_trace" in L.lib().mvs_last_error()


def test_a_valid_grabcut_call_gets_past_the_checks():
    assert _grabcut() in (0, E_NO_DEVICE)
    assert _grabcut(w=2, h=2, hl=0.0, hr=0.0, vl=0.0, vr=0.0) in (0, E_NO_DEVICE)            # a half image of one pixel
    assert _grabcut(hl=0.49, hr=0.49, gamma=100000.0, iters=1, max_rounds=1) in (0, E_NO_DEVICE)


def test_the_python_layer_checks_shapes():
    with pytest.raises(L.MvsError):
        P.GrabCutMasks(np.zeros((2, 8, 8), np.uint8))
    with pytest.raises(L.MvsError):
        P.GridMinCut(np.zeros((1, 3, 4), np.int32), np.zeros((1, 8, 4, 3), np.int32))
    with pytest.raises(L.MvsError) as e:
        P.LoadSequenceModels([], np.zeros((0, 2, 2, 3), np.uint8), np.zeros((0, 2, 2), np.float32), 1, 0, 1.0, masks=np.zeros((0, 2, 2), np.uint8),
                             segment=P.grabcut_params())
    assert "not both" in str(e.value)


# ---------------------------------------------------------------- the restatement ----
def _brute_force_g1(e, cap):
    """the union of the source sets of all minimum cuts of a tiny grid, by enumeration"""
    gh, gw = e.shape
    N = gw * gh
    ev = e.reshape(-1).astype(np.int64)
    arcs = [(i, int(nb.reshape(-1)[i]), int(cap[d].reshape(-1)[i])) for d in range(8) for ok, nb in [R.neighbour(gw, gh, d)]
            for i in range(N) if ok.reshape(-1)[i] and cap[d].reshape(-1)[i] > 0]
    best, union = None, 0
    for s in range(1 << N):
        v = sum(int(ev[i]) for i in range(N) if ev[i] > 0 and not s >> i & 1) + sum(int(-ev[i]) for i in range(N) if ev[i] < 0 and s >> i & 1)
        v += sum(c for i, j, c in arcs if s >> i & 1 and not s >> j & 1)
        if best is None or v < best:
            best, union = v, s
        elif v == best:
            union |= s
    return np.array([union >> i & 1 for i in range(N)], np.uint8).reshape(gh, gw)


@pytest.mark.parametrize("seed", range(6))
def test_g1_by_scipy_is_the_union_of_all_minimum_cuts(seed):
    rng = np.random.default_rng(seed)
    gw, gh = (4, 3) if seed % 2 else (3, 3)
    e = rng.integers(-4, 5, (gh, gw)).astype(np.int32)
    cap = rng.integers(0, 3, (8, gh, gw)).astype(np.int32)                 # small values: ties between cuts are the rule
    assert np.array_equal(R.g1_cut(e, cap), _brute_force_g1(e, cap))


def test_equal_capacities_have_many_minimum_cuts():
    """the 2-D tie case of the GPU tests: G1's maximal source set is everything up to the sink column, while the minimal one (what the
    source reaches in the residual graph = the complement of G1 on the reversed graph) is the source column alone"""
    e, cap = SC.equal_caps()
    gh, gw = e.shape
    want = R.g1_cut(e, cap)
    assert want[:, :-1].all() and not want[:, -1].any()
    rev = np.stack([np.where(ok, cap[d ^ 4].reshape(-1)[nb], 0) for d in range(8) for ok, nb in [R.neighbour(gw, gh, d)]]).astype(np.int32)
    minimal = 1 - R.g1_cut(-e, rev)
    assert minimal[:, 0].all() and not minimal[:, 1:].any()


def test_rule_12_is_where_a_linear_resize_at_2x_is_non_zero():
    rng = np.random.default_rng(3)
    for w, h in ((12, 10), (13, 11)):
        hw, hh = w // 2, h // 2
        m = (rng.random((hh, hw)) < 0.2).astype(np.float64)
        got = R.full_mask(m, w, h)
        # cv::resize INTER_LINEAR: source coordinate (x + 0.5) * (hw / w) - 0.5, neighbours clamped to the image
        def taps(n, hn):
            s = (np.arange(n) + 0.5) * (hn / n) - 0.5
            i0 = np.floor(s).astype(int)
            return np.clip(i0, 0, hn - 1), np.clip(i0 + 1, 0, hn - 1), s - i0
        if w % 2 == 0 and h % 2 == 0:                                      # exactly 2x: the stated equivalence
            xa, xb, fx = taps(w, hw)
            ya, yb, fy = taps(h, hh)
            lin = (m[np.ix_(ya, xa)] * (1 - fx)[None] + m[np.ix_(ya, xb)] * fx[None]) * (1 - fy)[:, None] + \
                  (m[np.ix_(yb, xa)] * (1 - fx)[None] + m[np.ix_(yb, xb)] * fx[None]) * fy[:, None]
            assert np.array_equal(got != 0, lin > 0)
        assert got.shape == (h, w) and set(np.unique(got)) <= {0, 255}
        assert (got[:2 * hh:2, :2 * hw:2][m != 0] == 255).all()


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_scene_conditions_and_restatement_properties(name):
    imgs, truth, p = SC.scene(name)
    kk = R.tlink_max(p["gamma"])
    for f, r in enumerate(SC.reference(name)):
        hh, hw = r["half"].shape[:2]
        assert (hw, hh) == (imgs.shape[2] // 2, imgs.shape[1] // 2)
        x0, y0, x1, y1 = r["rect"]
        assert 0 <= x0 < x1 <= hw and 0 <= y0 < y1 <= hh and (name != "border" or (x0 == 0 and y0 == 0))
        assert hw * hh * kk < 2 ** 31                                                         # scipy's int32 flow cannot overflow
        assert (r["cap"] >= 0).all() and r["cap"].max() <= 1024 * 50
        for d in range(8):                                                                    # rule 8: symmetric
            ok, nb = R.neighbour(hw, hh, d)
            assert np.array_equal(r["cap"][d][ok], r["cap"][d ^ 4].reshape(-1)[nb[ok]])
        assert r["labels0"].max() <= 4 and sorted(np.unique(r["labels0"][r["inside"]])) == [0, 1, 2, 3, 4]
        assert r["sums0"][:, :, 0].sum() == hw * hh and r["sums0"][0, :, 0].sum() == r["inside"].sum()
        for it in r["its"]:
            assert float(it["gap"].min()) >= 1e-9                                             # no pixel's component hangs on a last bit
            assert (np.abs(it["excess"]) <= kk).all() and (it["excess"][~r["inside"]] == -kk).all()
            assert not it["mask"][~r["inside"]].any() and it["mask"].any()                    # the cut exists and stays in the rectangle
            assert it["sums"][:, :, 0].sum() == hw * hh
        assert SC.iou(r["half_mask"], SC.half_truth(truth[f])) >= 0.9                         # the segmentation finds the ellipse
        assert SC.iou(r["mask"], truth[f]) >= SC.FULL_IOU_FLOOR                                # ... and rule 12 costs no more than its ring
        assert np.array_equal(r["mask"], R.full_mask(r["half_mask"], imgs.shape[2], imgs.shape[1]))


# ---------------------------------------------------------------- the shared rules as a program ----
def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "grabcut_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "grabcut_rules.cpp"), "-o", exe])
    return exe


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """tests/grabcut_rules.cpp: its own cases (an odd-sized image on heap blocks of exact size, a one-colour component, an empty model),
    then frame 0 of the odd-sized scene through the start and the restatement's second iteration, against the restatement: integers
    exactly, the links within the one unit that exp / log may move across llrint"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "grabcut rules ok" in run.stdout, run.stdout + run.stderr
    imgs, _, p = SC.scene("odd")
    r = SC.reference("odd")[0]
    h, w = imgs.shape[1:3]
    hh, hw = r["half"].shape[:2]
    N = hw * hh
    fg = r["its"][0]["mask"]                                                                  # iteration 2 starts from iteration 1's mask
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.asarray([w, h, 0], np.int32).tobytes())
        fh.write(np.asarray([p["hl"], p["hr"], p["vl"], p["vr"], p["gamma"]], np.float64).tobytes())
        fh.write(imgs[0].tobytes())
        fh.write(fg.astype(np.uint8).tobytes())
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    at = 0

    def take(dt, shape):
        nonlocal at
        a = np.frombuffer(raw, dt, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a
    half = take(np.uint32, (hh, hw))
    assert np.array_equal(np.stack([half & 255, half >> 8 & 255, half >> 16 & 255], axis=2), r["half"])
    assert int(take(np.int64, 1)[0]) == r["S"]
    assert np.abs(take(np.int32, (8, hh, hw)).astype(np.int64) - r["cap"]).max() <= 1
    assert np.array_equal(take(np.uint8, (hh, hw)), r["labels0"])
    assert np.array_equal(take(np.int64, (2, 5, 10)), r["sums0"])
    # the program's iteration used the models of ITS learn on the mask it was given; restate that here
    lab, gap = R.assign(R.fit_models(r["sums0"]), r["half"], fg)
    lab1 = take(np.uint8, (hh, hw))
    assert np.array_equal(lab1[gap >= 1e-9], lab[gap >= 1e-9])
    sums1 = take(np.int64, (2, 5, 10))
    assert np.array_equal(sums1, R.learn_sums(r["half"], fg, lab1))
    e, _ = R.excess_of(R.fit_models(sums1), r["half"], r["inside"], p["gamma"])
    assert np.abs(take(np.int32, (hh, hw)).astype(np.int64) - e).max() <= 1
    assert np.array_equal(take(np.uint8, (h, w)), R.full_mask(fg, w, h))
    assert at == len(raw)
