"""mvs_sift_detect on the GPU (csrc/sift.hip) against the numpy restatement tests/ref_sift.py: Gaussian levels and stage-6 candidates
bit for bit, final keys within FACTOR times the restatement's own float32 noise (tests/sift_scenes.py), batching, the device form,
max_features, capacity and run-to-run identity."""
import ctypes as C
import math

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import sift_scenes as SC

pytestmark = pytest.mark.gpu
NAMES = [s[0] for s in SC.SCENARIOS]


def cparams(p):
    return P.sift_params(**{k: v for k, v in p.items()})


def gpu_level(img, p, o, l):
    h, w = img.shape[:2]
    out = np.empty((2 * h) * (2 * w), np.float32)
    ow, oh = C.c_int32(), C.c_int32()
    prm = cparams(p)
    L.check(L.lib().mvs_test_sift_level(w, h, L.ptr(np.ascontiguousarray(img)), C.byref(prm), o, l, L.ptr(out), out.size, C.byref(ow), C.byref(oh)))
    return out[:ow.value * oh.value].reshape(oh.value, ow.value)


def gpu_candidates(imgs, p, cap=4096):
    n, h, w = imgs.shape[:3]
    off = np.zeros(n + 1, np.int64)
    ci, cf = np.zeros((cap, 4), np.int32), np.zeros((cap, 3), np.float32)
    prm = cparams(p)
    L.check(L.lib().mvs_test_sift_candidates(n, w, h, L.ptr(np.ascontiguousarray(imgs)), C.byref(prm), L.ptr(off), L.ptr(ci), L.ptr(cf), cap))
    return off, ci[:off[-1]], cf[:off[-1]]


@pytest.mark.parametrize("name", NAMES)
def test_gaussian_levels_are_bit_equal(name):
    img, p, pyr, _ = SC.reference(name)
    for o, g in enumerate(pyr):
        for l in range(g.shape[0]):
            got = gpu_level(img, p, o, l)
            assert got.shape == g[l].shape
            assert np.array_equal(got.view(np.uint32), g[l].view(np.uint32)), (name, o, l, float(np.abs(got - g[l]).max()))


@pytest.mark.parametrize("name", NAMES)
def test_stage6_candidates_are_bit_equal(name):
    img, p, _, ref = SC.reference(name)
    off, ci, cf = gpu_candidates(img[None], p)
    c = ref["cand"]
    assert off[1] == len(c["o"])
    assert np.array_equal(ci, np.stack([c["o"], c["l"], c["xi"], c["yi"]], 1).astype(np.int32))
    assert np.array_equal(cf[:, 0].view(np.uint32), c["x"].view(np.uint32)) and np.array_equal(cf[:, 1].view(np.uint32), c["y"].view(np.uint32))
    s_err = float(np.abs(cf[:, 2] / c["s"] - 1).max()) if len(ci) else 0.0
    print(f"{name}: {len(ci)} candidates, max relative scale difference {s_err:.2e} (bound {SC.FACTOR * SC.EPS_S:.1e})")
    assert s_err <= SC.FACTOR * SC.EPS_S


@pytest.mark.parametrize("name", NAMES)
def test_final_keys_within_the_restatement_noise(name):
    img, p, _, ref = SC.reference(name)
    keys, descs = P.DetectFeatureSingleView(img, cparams(p))
    off, ci, _ = gpu_candidates(img[None], p)
    c, n_cand = ref["cand"], len(ref["n_or"])
    clear = ref["margins"]["ori"] > SC.FACTOR * SC.EPS_H
    assert (~clear).sum() <= SC.MAX_UNCLEAR * max(1, n_cand)
    # the GPU's candidates are the restatement's (the test above), so the rows of a candidate are found by walking both in order:
    # a candidate whose margins clear must have the same number of orientations; an unclear one may differ by the noise
    assert len(ci) == n_cand
    if clear.all():
        assert len(keys) == len(ref["keys"])
    worst = dict(o=0.0, s=0.0, d=0.0)
    row = 0
    for i in range(n_cand):
        n_ref = int(ref["n_or"][i])
        if not clear[i]:
            # rows of this candidate on the GPU: those that share its x, y bit for bit
            n_gpu = 0
            while row + n_gpu < len(keys) and keys[row + n_gpu, 0] == c["x"][i] and keys[row + n_gpu, 1] == c["y"][i]:
                n_gpu += 1
            assert 1 <= n_gpu <= p["max_orient"]
            row += n_gpu
            continue
        for t in range(n_ref):
            k, r = keys[row + t], ref["keys"][ref["first"][i] + t]
            assert k[0] == r[0] and k[1] == r[1], (name, i, t, "a key above the bounds is missing or extra")
            do = abs(float(k[3]) - float(r[3]))
            worst["o"] = max(worst["o"], min(do, 2 * math.pi - do))
            worst["s"] = max(worst["s"], abs(float(k[2]) - float(r[2])) / float(r[2]))
            worst["d"] = max(worst["d"], float(np.abs(descs[row + t] - ref["descs"][ref["first"][i] + t]).max()))
            assert 0 <= k[3] < 2 * math.pi
        row += n_ref
    assert row == len(keys), "a key above the bounds is missing or extra"
    print(f"{name}: {len(keys)} keys; worst |do| {worst['o']:.2e} (bound {SC.FACTOR * SC.EPS_O:.1e}), |ds|/s {worst['s']:.2e} (bound {SC.FACTOR * SC.EPS_S:.1e}), "
          f"max |ddesc| {worst['d']:.2e} (bound {SC.FACTOR * SC.EPS_D:.1e})")
    assert worst["o"] <= SC.FACTOR * SC.EPS_O and worst["s"] <= SC.FACTOR * SC.EPS_S and worst["d"] <= SC.FACTOR * SC.EPS_D
    if len(descs):
        assert np.abs(np.linalg.norm(descs.astype(np.float64), axis=1) - 1).max() < 1e-6


def _five():
    _, w, h, fo, seed = SC.SCENARIOS[0]
    imgs = np.stack([SC.scene(w, h, seed), SC.scene(w, h, seed + 100), SC.scene(w, h, 0, black=True), SC.scene(w, h, seed + 200), SC.scene(w, h, seed + 300)])
    return imgs, SC.params_of(fo)


def test_five_lists_with_a_black_one_equal_five_calls_and_repeat():
    imgs, p = _five()
    keys, descs = P.DetectFeature(imgs, cparams(p))
    assert len(keys[2]) == 0 and sum(len(k) for k in keys) > 20
    for l in range(5):
        k1, d1 = P.DetectFeatureSingleView(imgs[l], cparams(p))
        assert k1.tobytes() == keys[l].tobytes() and d1.tobytes() == descs[l].tobytes(), l
    again = P.DetectFeature(imgs, cparams(p))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(keys + descs, again[0] + again[1]))


def test_the_device_form_on_a_side_stream_equals_the_host_form():
    import torch
    imgs, p = _five()
    keys, descs = P.DetectFeature(imgs, cparams(p))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = torch.from_numpy(imgs).cuda()
        off, tk, td = P.DetectFeature(t, cparams(p), stream=st.cuda_stream)
    st.synchronize()
    assert list(np.diff(off)) == [len(k) for k in keys]
    assert tk.cpu().numpy().tobytes() == np.concatenate(keys).tobytes() and td.cpu().numpy().tobytes() == np.concatenate(descs).tobytes()


def test_max_features_keeps_the_first_keys_and_capacity_reports_the_need():
    imgs, p = _five()
    keys, descs = P.DetectFeature(imgs, cparams(p))
    cut = min(len(k) for i, k in enumerate(keys) if i != 2) - 2
    assert cut >= 1
    k2, d2 = P.DetectFeature(imgs, cparams(dict(p, max_features=cut)))
    for l in range(5):
        assert k2[l].tobytes() == keys[l][:cut].tobytes() and d2[l].tobytes() == descs[l][:cut].tobytes()
    total = sum(len(k) for k in keys)
    off = np.full(6, -1, np.int64)
    kb, db = np.empty((total - 1, 4), np.float32), np.empty((total - 1, 128), np.float32)
    prm = cparams(p)
    rc = L.lib().mvs_sift_detect(5, imgs.shape[2], imgs.shape[1], L.ptr(imgs), C.byref(prm), L.ptr(off), L.ptr(kb), L.ptr(db), total - 1)
    assert rc == -1 and list(np.diff(off)) == [len(k) for k in keys] and off[0] == 0


def test_load_sequence_models_with_sift_detects_on_its_views_and_culls():
    """the Python layer only: keys / descs of LoadSequenceModels(sift=...) are DetectFeature on the views it generated followed by
    CullKeypoints, list by list; without ``sift`` the result is what it was"""
    from multiviewstitch_amd import scene as S
    from tests.test_views_host import CFRAMES, CH, CVIEWS, CW
    cams, depths = S.make_sequence(CFRAMES, CW, CH, 25.0, f=2.2)
    imgs = np.stack([SC.scene(CW, CH, 40 + i) for i in range(CFRAMES)])
    prm = P.sift_params(hl=0.05, vr=0.05)
    plain = P.LoadSequenceModels(cams, imgs, depths, CVIEWS, 0, 10.0)
    assert "keys" not in plain and "descs" not in plain
    seq = P.LoadSequenceModels(cams, imgs, depths, CVIEWS, 0, 10.0, sift=prm, min_dsp=S.MIN_DSP, max_dsp=S.MAX_DSP)
    assert np.array_equal(seq["views"], plain["views"]) and np.array_equal(seq["tex"], plain["tex"])
    keys, descs = P.DetectFeature(plain["views"], prm)
    assert len(keys) == CFRAMES * CVIEWS and sum(len(k) for k in keys) > 50
    ck, cd = P.CullKeypoints(cams, plain["depths"], plain["tex"], keys, descs, S.MIN_DSP, S.MAX_DSP)
    assert 0 < sum(len(k) for k in ck) <= sum(len(k) for k in keys)
    for l in range(len(keys)):
        assert seq["keys"][l].tobytes() == ck[l].tobytes() and seq["descs"][l].tobytes() == cd[l].tobytes()


def test_the_chain_from_images_to_matches_equals_the_restatement_chain():
    """LoadSequenceModels(sift=...) on the 96 x 72 three-frame cull scenario, loaded as two sequences (views 10 and 6 degrees apart), then
    MatchFeature on the GPU, against ref_views -> ref_sift -> the cull of ref_views -> ref_match (tests/sift_scenes.py
    chain_reference).  The scenario clears every margin (tests/test_sift_host.py), so the raw rows are equal element for element."""
    from multiviewstitch_amd import scene as S
    from tests.test_views_host import CVIEWS
    q = SC.chain_reference()
    assert q["unclear"] == 0 and q["ori_unclear"] == 0
    prm = cparams(q["sift"])
    loaded = []
    for ref in q["seqs"]:
        seq = P.LoadSequenceModels(q["cameras"], q["imgs"], q["depths"], CVIEWS, 0, ref["rot"], sift=prm, min_dsp=S.MIN_DSP, max_dsp=S.MAX_DSP)
        assert np.array_equal(np.asarray(seq["views"]).reshape(ref["views"].shape), ref["views"])
        assert np.array_equal(np.asarray(seq["tex"]).reshape(ref["tex"].shape), ref["tex"])
        worst = 0.0
        for l, (k, d) in enumerate(zip(seq["keys"], seq["descs"])):
            assert k.shape == ref["keys"][l].shape and np.array_equal(k[:, :2], ref["keys"][l][:, :2]), (ref["rot"], l)
            worst = max(worst, float(np.abs(d - ref["descs"][l]).max(initial=0.0)))
        print(f"views {ref['rot']} degrees apart: {sum(len(k) for k in seq['keys'])} keys after the cull, max |ddesc| {worst:.2e} (bound {SC.FACTOR * SC.CHAIN_EPS_D:.1e})")
        assert worst <= SC.FACTOR * SC.CHAIN_EPS_D
        loaded.append(seq)
    a, b = loaded
    got = P.MatchFeature(a["keys"], a["descs"], b["keys"], b["descs"], CVIEWS)
    want = q["raw"]
    print("matches per frame pair", [[len(w) for w in row] for row in want])
    assert len(got) == len(want) and sum(len(w) for row in want for w in row) >= 9 * SC.CHAIN_MIN_MATCHES
    for i, row in enumerate(want):
        for j, w in enumerate(row):
            assert got[i][j].dtype == np.int32 and np.array_equal(got[i][j], w), (i, j, len(got[i][j]), len(w))
