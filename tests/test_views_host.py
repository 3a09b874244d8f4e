"""Host side of mvs_gen_new_views(_dev) and mvs_keypoint_cull(_dev) (include/mvs.h): the argument checks, which run before any
device is needed, and the scenarios of tests/test_gpu_views.py, checked here from the restatement's diagnostics (tests/ref_views.py)
to hold what they are there for."""
import ctypes as C
import functools
import math

import numpy as np

from multiviewstitch_amd import _lib
from multiviewstitch_amd import scene as S
from tests import ref_views as RV

E_INVALID = -1


def yawed_camera(w, h, yaw=0.3):
    """fx = fy = 1.2 w, the principal point at the centre, the camera yawed by `yaw` rad"""
    c, s = math.cos(yaw), math.sin(yaw)
    return S.Camera(1.2 * w, 1.2 * w, w / 2 - 0.5, h / 2 - 0.5, np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]), np.zeros(3), w, h)


# name -> (w, h, view_count, axis, rot_angle)
SCENARIOS = {"integer_offsets": (96, 72, 3, 0, 10.0), "odd_even": (97, 71, 4, 1, 7.5), "equal_branches": (64, 48, 3, 0, 10.0),
             "wide": (64, 48, 3, 0, 60.0)}


@functools.lru_cache(maxsize=None)
def view_scenario(name):
    """-> (cameras [1], imgs [1, h, w, 3], view_count, axis, rot_angle, (views, tex, diagnostics) of the restatement)"""
    w, h, vc, axis, rot = SCENARIOS[name]
    cams = [yawed_camera(w, h)]
    imgs = np.random.default_rng(sorted(SCENARIOS).index(name)).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    return cams, imgs, vc, axis, rot, RV.gen_new_views(cams, imgs, vc, axis, rot)


def test_the_view_scenarios_hold_what_they_should():
    diag = {name: view_scenario(name)[5][2][0] for name in SCENARIOS}
    for name, ds in diag.items():
        for k, d in enumerate(ds):
            print(name, k, {a: b for a, b in d.items() if a != "branch_map"})
    d = diag["integer_offsets"]                                    # views 0 and 2: integer offsets in both directions
    for k in (0, 2):
        assert d[k]["offsetx"] == int(d[k]["offsetx"]) and d[k]["offsety"] == int(d[k]["offsety"])
    assert (d[0]["colliding"], d[2]["colliding"]) == (106, 112) and max(q["max_writers"] for q in d) == 4
    d = diag["odd_even"]                                           # 4 views: -15, -7.5, 0, 7.5; 22.5 is never used
    assert RV.angles(4, 7.5) == [-15.0, -7.5, 0.0, 7.5]
    assert all(d[k]["colliding"] > 0 for k in (0, 1, 3))
    assert all(66 <= d[k]["branches"][RV.V_EQUAL] <= 77 for k in (0, 1, 3))
    d = diag["equal_branches"]
    assert d[1]["branches"][RV.BOTH_EQUAL] == 882 and d[1]["branches"][RV.U_EQUAL] == 2016
    d = diag["wide"]
    assert sum(q["wf_nonpositive"] for q in d) > 0 and any(q["in_range"] == 0 for q in d)      # a view with no pixel in range: the 1e9 offsets
    for b in range(4):                                             # every branch is hit somewhere
        assert sum(q["branches"][b] for ds in diag.values() for q in ds) > 0, b
    for name in ("integer_offsets", "odd_even", "equal_branches"):
        w, h = SCENARIOS[name][:2]
        for q in diag[name]:
            assert 0.85 * w * h <= q["painted"] <= w * h, (name, q["painted"] / (w * h))


# ----------------------------------------------------------------- cull scenario ----
CW, CH, CVIEWS, CFRAMES = 96, 72, 3, 3
EMPTY_LIST, ALL_REMOVED_LIST, LARGE_LIST = 4, 7, 2


@functools.lru_cache(maxsize=1)
def cull_scenario():
    """3 frames at 96 x 72 on a ring around scene.py's surface, 25 degrees apart, with a lens long enough (fx = 2.2 w) for the surface
    to overflow the image, so points near an image's edge leave the other frames; tex from the restatement.  9 key lists: random positions from 3 pixels
    outside the image on every side, fractional; list 2 holds 5 000, list 4 is empty, list 7 holds only keys the cull removes; two
    keys are NaN / inf.  -> dict(cameras, depths, tex, keys, descs, masks)"""
    cams, depths = S.make_sequence(CFRAMES, CW, CH, 25.0, f=2.2)
    rng = np.random.default_rng(8)
    imgs = rng.integers(0, 256, (CFRAMES, CH, CW, 3), dtype=np.uint8)
    _, tex, _ = RV.gen_new_views(cams, imgs, CVIEWS, 0, 10.0)
    masks = (rng.random((CFRAMES, CH * CW)) < 0.7).astype(np.uint8)
    keys = []
    for i in range(CFRAMES * CVIEWS):
        n = {EMPTY_LIST: 0, LARGE_LIST: 5000}.get(i, 300 + 37 * i)
        k = np.stack([rng.uniform(-3, CW + 3, n), rng.uniform(-3, CH + 3, n), rng.uniform(1, 8, n), rng.uniform(-3.2, 3.2, n)], 1).astype(np.float32)
        keys.append(k)
    keys[0][5, 0], keys[0][6, 1] = np.nan, np.inf
    what, _, _ = RV.keypoint_cull(cams, CVIEWS, keys, None, tex, depths, S.MIN_DSP, S.MAX_DSP)
    keys[ALL_REMOVED_LIST] = keys[ALL_REMOVED_LIST][what[ALL_REMOVED_LIST] != RV.SURVIVOR]
    descs = [rng.normal(size=(len(k), 128)).astype(np.float32) for k in keys]
    return dict(cameras=cams, depths=depths.reshape(CFRAMES, -1), tex=tex, keys=keys, descs=descs, masks=masks, imgs=imgs)


@functools.lru_cache(maxsize=2)
def cull_expected(masked):
    q = cull_scenario()
    return RV.keypoint_cull(q["cameras"], CVIEWS, q["keys"], q["descs"], q["tex"], q["depths"], S.MIN_DSP, S.MAX_DSP, q["masks"] if masked else None)


def test_the_cull_scenario_holds_every_category():
    q = cull_scenario()
    what, keys_out, _ = cull_expected(False)
    allw = np.concatenate(what)
    counts = {c: int((allw == c).sum()) for c in range(6)}
    print("cull categories", counts, "per list", [len(k) for k in keys_out])
    for c in (RV.SURVIVOR, RV.OUTSIDE, RV.UNMAPPED, RV.INVALID, RV.LEAVES):
        assert counts[c] > 0, c
    allk = np.concatenate(q["keys"])
    assert (allk[:, :2] != np.trunc(allk[:, :2])).any() and not np.isfinite(allk[:, :2]).all()
    assert len(q["keys"][EMPTY_LIST]) == 0 and len(q["keys"][LARGE_LIST]) == 5000
    assert len(q["keys"][ALL_REMOVED_LIST]) > 0 and len(keys_out[ALL_REMOVED_LIST]) == 0
    mwhat, mkeys, _ = cull_expected(True)
    assert (np.concatenate(mwhat) == RV.MASKED).sum() > 0
    assert sum(len(k) for k in mkeys) < sum(len(k) for k in keys_out)


# ------------------------------------------------------------- argument checks ----
W, H, VIEWS, N = 8, 6, 2, 2


def _cams(n=N, w=W, h=H):
    cam = S.Camera(10.0, 10.0, w / 2 - 0.5, h / 2 - 0.5, np.eye(3), np.zeros(3), w, h)
    return (_lib.CCamera * n)(*[_lib.CCamera.of(cam)] * n)


def test_the_four_symbols_are_exported():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("mvs_gen_new_views", "mvs_gen_new_views_dev", "mvs_keypoint_cull", "mvs_keypoint_cull_dev"):
        assert hasattr(lib, name) and name in _lib.EXPORTS


def _views_call(dev, **kw):
    a = dict(n=N, cams=_cams(), imgs=np.zeros((N, H, W, 3), np.uint8), vc=VIEWS, axis=0, rot=10.0, views=np.zeros((N, VIEWS, H, W, 3), np.uint8),
             tex=np.zeros((N, VIEWS, H * W), np.int32))
    a.update(kw)
    P = _lib.ptr
    common = (a["n"], a["cams"], P(a["imgs"]), a["vc"], a["axis"], a["rot"], P(a["views"]), P(a["tex"]))
    L = _lib.lib()
    return L.mvs_gen_new_views_dev(*common, None) if dev else L.mvs_gen_new_views(*common)


def test_gen_new_views_rejects_bad_arguments_without_a_device():
    mixed = _cams()
    mixed[1].w = W + 1
    cases = [dict(vc=0), dict(vc=-2), dict(axis=-1), dict(axis=3), dict(n=0), dict(n=-1), dict(cams=mixed), dict(cams=None), dict(imgs=None),
             dict(views=None), dict(tex=None), dict(cams=_cams(w=65536)), dict(cams=_cams(h=65536))]
    for dev in (False, True):
        for kw in cases:
            assert _views_call(dev, **kw) == E_INVALID, (dev, kw)
            assert _lib.lib().mvs_last_error()
        assert _views_call(dev) != E_INVALID                        # (no device: MVS_E_NO_DEVICE)


def _cull_call(dev, **kw):
    total = 5
    a = dict(n=N, vc=VIEWS, cams=_cams(), off=np.array([0, 2, 2, 4, 5], np.int64), keys=np.ones((total, 4), np.float32),
             descs=np.zeros((total, 128), np.float32), tex=np.zeros((N, VIEWS, H * W), np.int32), depths=np.full((N, H * W), 0.1, np.float32),
             mask=np.ones((N, H * W), np.uint8), keep=np.zeros(total, np.uint8), ooff=np.zeros(N * VIEWS + 1, np.int64),
             okeys=np.zeros((total, 4), np.float32), odescs=np.zeros((total, 128), np.float32))
    a.update(kw)
    P = _lib.ptr
    common = (a["n"], a["vc"], a["cams"], P(a["off"]), P(a["keys"]), P(a["descs"]), P(a["tex"]), P(a["depths"]), 0.0025, 0.3, P(a["mask"]),
              P(a["keep"]), P(a["ooff"]), P(a["okeys"]), P(a["odescs"]))
    L = _lib.lib()
    return L.mvs_keypoint_cull_dev(*common, None) if dev else L.mvs_keypoint_cull(*common)


def test_keypoint_cull_rejects_bad_arguments_without_a_device():
    mixed = _cams()
    mixed[1].h = H + 2
    cases = [dict(n=0), dict(vc=0), dict(cams=None), dict(cams=mixed), dict(cams=_cams(w=65536)), dict(off=None), dict(off=np.array([1, 2, 2, 4, 5], np.int64)),
             dict(off=np.array([0, 3, 2, 4, 5], np.int64)), dict(keys=None), dict(tex=None), dict(depths=None), dict(ooff=None), dict(okeys=None),
             dict(odescs=None)]
    for dev in (False, True):
        for kw in cases:
            assert _cull_call(dev, **kw) == E_INVALID, (dev, kw)
            assert _lib.lib().mvs_last_error()
        for kw in (dict(), dict(descs=None, odescs=None), dict(mask=None), dict(keep=None)):      # the optional ones
            assert _cull_call(dev, **kw) != E_INVALID, (dev, kw)
