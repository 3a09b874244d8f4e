"""Host side of mvs_sift_detect (include/mvs.h): symbols, the layout of mvs_sift_params, the argument checks (they run before a device
is needed), properties of the numpy restatement tests/ref_sift.py, the rounding noise that sizes the GPU tolerances
(tests/sift_scenes.py), and the host rules (csrc/sift_rules.h) as a stand-alone program under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import ref_sift as R, sift_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def _call(n=1, w=16, h=16, imgs=True, off=True, keys=True, descs=True, prm=True, cap=8, **fields):
    img = np.zeros((max(n, 1), h if 0 < h < 100 else 16, w if 0 < w < 100 else 16, 3), np.uint8)
    o, k, d = np.zeros(max(n, 1) + 1, np.int64), np.zeros((8, 4), np.float32), np.zeros((8, 128), np.float32)
    p = P.sift_params(**fields)
    return L.lib().mvs_sift_detect(n, w, h, L.ptr(img) if imgs else None, C.byref(p) if prm else None, L.ptr(o) if off else None,
                                   L.ptr(k) if keys else None, L.ptr(d) if descs else None, cap)


def test_symbols_and_params_layout():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_sift_default_params", "mvs_sift_detect", "mvs_sift_detect_dev", "mvs_test_sift_level", "mvs_test_sift_candidates"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert C.sizeof(L.CSiftParams) == 64 and L.CSiftParams.hl.offset == 32 and L.CSiftParams.dog_threshold.offset == 16
    p = P.sift_params()
    assert (p.first_octave, p.dog_levels, p.max_orient, p.max_features) == (-1, 3, 2, 2 ** 31 - 1)
    assert (p.dog_threshold, p.edge_threshold, p.sigma0, p.sigma_in) == tuple(float(np.float32(v)) for v in (0.02, 10, 1.6, 0.5))
    assert (p.hl, p.hr, p.vl, p.vr) == (0, 0, 0, 0)


BAD = [dict(imgs=False), dict(off=False), dict(keys=False), dict(descs=False), dict(prm=False), dict(n=0), dict(w=7), dict(h=7), dict(w=65536),
       dict(h=65536), dict(first_octave=1), dict(first_octave=-2), dict(dog_levels=0), dict(dog_levels=6), dict(max_orient=0), dict(max_orient=5),
       dict(max_features=0), dict(hl=-0.1), dict(hr=1.0), dict(vl=math.nan), dict(vr=1.5), dict(hl=0.5, hr=0.5), dict(vl=0.7, vr=0.4),
       dict(dog_threshold=math.inf), dict(edge_threshold=math.nan), dict(sigma0=math.inf), dict(sigma_in=math.nan), dict(sigma0=0.9),
       dict(sigma0=40.0), dict(cap=-1)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD])
def test_argument_errors_need_no_device(kw):
    assert _call(**kw) == E_INVALID
    assert b"mvs_sift_detect" in L.lib().mvs_last_error()


def test_the_device_form_rejects_misaligned_outputs_without_a_device():
    img, off, p = np.zeros((1, 16, 16, 3), np.uint8), np.zeros(2, np.int64), P.sift_params()
    buf = np.zeros(8 * 132 + 8, np.float32)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    for keys, descs in ((a + 4, a + 64), (a, a + 64 + 8)):
        assert L.lib().mvs_sift_detect_dev(1, 16, 16, L.ptr(img), C.byref(p), L.ptr(off), L.ptr(keys), L.ptr(descs), 8, None) == E_INVALID
        assert b"16-byte aligned" in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    assert _call() in (0, -4)                                   # MVS_E_NO_DEVICE without a GPU


def _grey_img(a):
    g = np.clip(np.asarray(a) * 255, 0, 255).astype(np.uint8)
    return np.stack([g, g, g], -1)


def _blob(w, h, cx, cy, s, amp=0.4):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return _grey_img(0.3 + amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s)))


def test_constant_and_margin_blacked_images_give_no_keys():
    assert len(R.detect(np.full((24, 32, 3), 117, np.uint8))["keys"]) == 0
    img = np.zeros((40, 48, 3), np.uint8)
    img[:, :12] = SC.scene(48, 40, 5)[:, :12]                     # all content inside the left margin
    p = R.default_params(hl=0.25)
    assert len(R.detect(img, R.default_params())["keys"]) > 0 and len(R.detect(img, p)["keys"]) == 0


def test_one_blob_gives_one_key_where_the_float64_restatement_puts_it():
    cx, cy, s = 23.3, 19.6, 3.0
    img = _blob(48, 40, cx, cy, s)
    a, b = R.detect(img, dt=np.float32), R.detect(img, dt=np.float64)
    assert len(a["n_or"]) == 1 and len(b["n_or"]) == 1
    ka, kb = a["keys"][0].astype(np.float64), b["keys"][0]
    assert abs(ka[0] - kb[0]) < 1e-3 and abs(ka[1] - kb[1]) < 1e-3 and abs(ka[2] / kb[2] - 1) < 1e-3
    # recorded, not fixed: the pixel centre of (cx, cy) is (cx + 0.5, cy + 0.5) in key coordinates; one 3 x 3 solve does not converge fully
    print(f"blob at ({cx + 0.5}, {cy + 0.5}), sigma {s}: key ({kb[0]:.4f}, {kb[1]:.4f}), s {kb[2]:.4f}; "
          f"distance {math.hypot(kb[0] - cx - 0.5, kb[1] - cy - 0.5):.4f} px")
    assert math.hypot(kb[0] - cx - 0.5, kb[1] - cy - 0.5) < 1.0


def test_a_shift_by_two_to_the_octaves_shifts_the_keys_with_equal_descriptors():
    w, h = 96, 80
    p = R.default_params()
    shift = 2 ** R.octaves(2 * w, 2 * h)                          # every octave grid of the doubled image moves by whole pixels
    base = np.zeros((h, w))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for cx, cy, s, amp in ((30.3, 30.2, 2.0, 0.4), (44.1, 47.7, 3.1, -0.25), (36.5, 40.0, 1.5, 0.3)):
        base += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    g = np.clip((0.4 + base) * 255, 0, 255).astype(np.uint8)
    g[np.abs(base) < 2e-3] = 102                                  # a flat background: the replicated border carries nothing
    a = R.detect(np.stack([g, g, g], -1), p)
    gs = np.full_like(g, 102)
    gs[:, shift:] = g[:, :-shift]
    b = R.detect(np.stack([gs, gs, gs], -1), p)
    assert len(a["keys"]) >= 3 and len(a["keys"]) == len(b["keys"])
    assert np.array_equal(a["keys"][:, 1:], b["keys"][:, 1:]) and np.array_equal(a["keys"][:, 0] + np.float32(shift), b["keys"][:, 0])
    assert np.array_equal(a["descs"], b["descs"])


def test_descriptors_have_unit_norm():
    _, _, _, ref = SC.reference("64x48_up")
    n = np.linalg.norm(ref["descs"].astype(np.float64), axis=1)
    assert len(n) > 10 and np.abs(n - 1).max() < 1e-6 and ref["descs"].min() >= 0


def test_matches_across_a_view_change_agree_with_the_tex_table():
    """the views of ref_views 10 degrees apart (the first sequence of the chain scenario), all keys of the restatement after the cull,
    matched with ref_match: the tex tables take both keys of a match back to the frame's own raster, where a right match meets within
    2 pixels (a match that does not is a wrong or a coarse-octave one; it is printed, SIFT promises none).  The counts are recorded (profiles/r12/sift.md) and only choose the scenario: every pair of views of a frame has at least
    CHAIN_MIN_MATCHES such matches."""
    from multiviewstitch_amd import scene as S
    from tests import ref_match as RM, ref_views as RV
    from tests.test_views_host import CFRAMES, CH, CVIEWS, CW
    q = SC.chain_reference()
    ref = dict(q["seqs"][0])
    p = dict(q["sift"], max_features=2 ** 31 - 1)                   # every key of a view, not the first 12 the chain keeps
    det = [R.detect(v, p) for v in ref["views"].reshape(-1, CH, CW, 3)]
    _, ref["keys"], ref["descs"] = RV.keypoint_cull(q["cameras"], CVIEWS, [d["keys"] for d in det], [d["descs"] for d in det], ref["tex"], q["depths"],
                                                    S.MIN_DSP, S.MAX_DSP)
    for f in range(CFRAMES):
        for va, vb in ((0, 1), (1, 2), (0, 2)):
            la, lb = f * CVIEWS + va, f * CVIEWS + vb
            m = RM.match_pair(ref["descs"][la], ref["descs"][lb])
            ka, kb = ref["keys"][la][m[:, 0]].astype(np.float64), ref["keys"][lb][m[:, 1]].astype(np.float64)
            ia = ref["tex"][f, va, RV.cvt_i32(ka[:, 1]) * CW + RV.cvt_i32(ka[:, 0])].astype(np.int64)
            ib = ref["tex"][f, vb, RV.cvt_i32(kb[:, 1]) * CW + RV.cvt_i32(kb[:, 0])].astype(np.int64)
            assert (ia >= 0).all() and (ib >= 0).all()                # the cull kept only keys on mapped pixels
            dist = np.hypot(ia % CW - ib % CW, ia // CW - ib // CW)
            good = int((dist <= 2).sum())
            print(f"frame {f}, views {va} and {vb} ({(vb - va) * ref['rot']:g} degrees): {len(ref['keys'][la])} and {len(ref['keys'][lb])} keys, "
                  f"{len(m)} matches, {good} within 2 px on the frame's raster, worst {dist.max(initial=0.0):.2f} px")
            assert good >= SC.CHAIN_MIN_MATCHES


def test_the_chain_scenario_clears_every_margin():
    """every orientation decision in front of the max_features cut clears FACTOR * CHAIN_EPS_H, no match of the two sequences can be
    gained or lost by descriptors within FACTOR * CHAIN_EPS_D of the restatement's (sift_scenes.match_unclear), and the noise of the
    restatement on these 18 views (larger than on the small scenarios: painted views have hard edges) stays inside the two constants;
    the chain compares no orientation or scale"""
    q = SC.chain_reference()
    print("chain scenario: match decisions that could flip", q["unclear"], "orientation decisions below the bound", q["ori_unclear"],
          "matches", int(q["counts"].sum()), "keys per list", [[len(k) for k in s["keys"]] for s in q["seqs"]])
    assert q["unclear"] == 0 and q["ori_unclear"] == 0
    worst = dict(eps_d=0.0, eps_h=0.0)
    for s in q["seqs"]:
        for v in s["views"].reshape((-1,) + s["views"].shape[-3:]):
            n = R.noise(v, q["sift"])
            worst = {k: max(worst[k], n[k]) for k in worst}
    print("noise on the chain's views", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["eps_d"] <= SC.CHAIN_EPS_D and worst["eps_h"] <= SC.CHAIN_EPS_H


def test_match_unclear_counts_a_match_at_the_threshold_and_none_far_from_it():
    """the interval rule itself: orthogonal unit descriptors matched with themselves are decided; a second descriptor placed so that
    dist = ratiomax * dist2 within the noise is not"""
    d = np.zeros((3, 128), np.float32)
    d[0, :4], d[1, 4:8], d[2, 8:12] = 0.5, 0.5, 0.5
    assert SC.match_unclear(d, d, SC.FACTOR * SC.EPS_D) == 0
    from tests import ref_match as RM
    t = np.zeros((1, 128), np.float32)
    t[0, :4] = 0.5
    lo, hi = 0.0, 0.5
    for _ in range(40):                                               # bisect the weight at which the second best spoils the ratio test
        mid = (lo + hi) / 2
        c = np.zeros((2, 128), np.float32)
        c[0, :4], c[1, :4], c[1, 4:8] = 0.5, mid, math.sqrt(max(0.0, 0.25 - mid * mid))
        lo, hi = (mid, hi) if len(RM.match_pair(t, c)) else (lo, mid)
    c[1, :4], c[1, 4:8] = lo, math.sqrt(0.25 - lo * lo)
    assert SC.match_unclear(t, c, SC.FACTOR * SC.EPS_D) > 0


def test_stage_1_to_4_arithmetic_against_plain_loops():
    """24 x 16, first octave doubled: the base image and the first Gaussian level, sample by sample with float32 scalars"""
    img = SC.scene(24, 16, 3)
    p = R.default_params(hl=0.1, vr=0.2)
    f = np.float32
    l_, r_, t_, b_ = R.margins_px(24, 16, p)
    I = [[f(0) if (x < l_ or x >= r_ or y < t_ or y >= b_) else f(int(R.grey8(img[y, x]))) / f(255) for x in range(24)] for y in range(16)]
    rowv = lambda y, X: I[y][X // 2] if X % 2 == 0 else f(0.5) * (I[y][X // 2] + I[y][min(X // 2 + 1, 23)])
    U = [[rowv(Y // 2, X) if Y % 2 == 0 else f(0.5) * (rowv(Y // 2, X) + rowv(min(Y // 2 + 1, 15), X)) for X in range(48)] for Y in range(32)]
    assert np.array_equal(np.array(U, f), R.base(R.grey(img, p, f), p, f))
    r, k = R.taps(R.level_sigma(0, p))
    cl = lambda v, n: min(max(v, 0), n - 1)
    rows = [[None] * 48 for _ in range(32)]
    for Y in range(32):
        for X in range(48):
            acc = k[0] * U[Y][cl(X - r, 48)]
            for i in range(1, 2 * r + 1):
                acc = acc + k[i] * U[Y][cl(X - r + i, 48)]
            rows[Y][X] = acc
    g0 = R.pyramid(img, p, f)[0][0]
    for Y in (0, 1, 7, 30, 31):
        for X in (0, 2, 23, 46, 47):
            acc = k[0] * rows[cl(Y - r, 32)][X]
            for i in range(1, 2 * r + 1):
                acc = acc + k[i] * rows[cl(Y - r + i, 32)][X]
            assert acc == g0[Y, X] and type(acc) is np.float32


def test_stage_5_and_6_arithmetic_against_plain_loops():
    img, p, pyr, ref = SC.reference("64x48")
    f = np.float32
    T, e = f(p["dog_threshold"]) / f(p["dog_levels"]), f(p["edge_threshold"])
    found = []
    for o, g in enumerate(pyr):
        d = g[1:] - g[:-1]
        for l in range(1, p["dog_levels"] + 1):
            for y in range(1, d.shape[1] - 1):
                for x in range(1, d.shape[2] - 1):
                    v = d[l, y, x]
                    if not abs(v) > T:
                        continue
                    nb = [d[l + a, y + b, x + c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
                    if not (all(v > u for u in nb) or all(v < u for u in nb)):
                        continue
                    D = d[l - 1:l + 2, y - 1:y + 2, x - 1:x + 2]
                    gx, gy, gs = f(.5) * (D[1, 1, 2] - D[1, 1, 0]), f(.5) * (D[1, 2, 1] - D[1, 0, 1]), f(.5) * (D[2, 1, 1] - D[0, 1, 1])
                    dxx, dyy, dss = (D[1, 1, 2] + D[1, 1, 0]) - f(2) * v, (D[1, 2, 1] + D[1, 0, 1]) - f(2) * v, (D[2, 1, 1] + D[0, 1, 1]) - f(2) * v
                    dxy = f(.25) * ((D[1, 2, 2] - D[1, 2, 0]) - (D[1, 0, 2] - D[1, 0, 0]))
                    dxs = f(.25) * ((D[2, 1, 2] - D[2, 1, 0]) - (D[0, 1, 2] - D[0, 1, 0]))
                    dys = f(.25) * ((D[2, 2, 1] - D[2, 0, 1]) - (D[0, 2, 1] - D[0, 0, 1]))
                    tr, det2 = dxx + dyy, dxx * dyy - dxy * dxy
                    if not (det2 > 0 and (tr * tr) * e < ((e + f(1)) * (e + f(1))) * det2):
                        continue
                    b0, b1, b2 = -gx, -gy, -gs
                    det = (dxx * (dyy * dss - dys * dys) - dxy * (dxy * dss - dys * dxs)) + dxs * (dxy * dys - dyy * dxs)
                    if det == 0:
                        continue
                    dx = ((b0 * (dyy * dss - dys * dys) - dxy * (b1 * dss - dys * b2)) + dxs * (b1 * dys - dyy * b2)) / det
                    dy = ((dxx * (b1 * dss - dys * b2) - b0 * (dxy * dss - dys * dxs)) + dxs * (dxy * b2 - b1 * dxs)) / det
                    ds = ((dxx * (dyy * b2 - b1 * dys) - dxy * (dxy * b2 - b1 * dxs)) + b0 * (dxy * dys - dyy * dxs)) / det
                    if not (abs(dx) < 1 and abs(dy) < 1 and abs(ds) < 1) or not abs(v + f(.5) * ((gx * dx + gy * dy) + gs * ds)) > T:
                        continue
                    step = f(R.step_of(o, p))
                    found.append((o, l, x, y, ((f(x) + dx) + f(.5)) * step, ((f(y) + dy) + f(.5)) * step))
    c = ref["cand"]
    assert len(found) == len(c["o"]) > 5
    for i, (o, l, x, y, kx, ky) in enumerate(found):
        assert (o, l, x, y) == (c["o"][i], c["l"][i], c["xi"][i], c["yi"][i]) and kx == c["x"][i] and ky == c["y"][i]


def test_the_noise_estimates_stay_inside_the_named_constants():
    """float32 against float64 of the restatement on the GPU scenarios: the EPS_* of tests/sift_scenes.py bound what is measured here,
    every candidate is present in both runs, and at most MAX_UNCLEAR of a scenario's candidates sit below the orientation bound"""
    for name, w, h, fo, seed in SC.SCENARIOS:
        img, p, _, ref = SC.reference(name)
        n = R.noise(img, p)
        mo = ref["margins"]["ori"]
        print(name, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in n.items()}, "candidates", len(mo), "keys", len(ref["keys"]),
              "smallest orientation margin", f"{mo.min():.2e}" if len(mo) else "-")
        assert n["n"] == n["n32"] == n["n64"] >= 1
        assert n["eps_o"] <= SC.EPS_O and n["eps_d"] <= SC.EPS_D and n["eps_s"] <= SC.EPS_S and n["eps_h"] <= SC.EPS_H
        assert (mo <= SC.FACTOR * SC.EPS_H).sum() <= SC.MAX_UNCLEAR * len(mo)
    assert (SC.reference("64x48_up")[3]["n_or"] == 2).any()      # the key with two orientations


def test_the_host_rules_under_the_sanitizers(tmp_path):
    """tests/sift_rules.cpp: octave counts, tap tables and sift_refine as host code, compiled without the device pass and run as a
    program of its own"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "sift_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "sift_rules.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "sift rules ok" in run.stdout, run.stdout + run.stderr
