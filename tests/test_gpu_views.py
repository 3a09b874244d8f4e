"""Image3D::GenNewViews and the background cull of the key points on the GPU (R/Image3D/Image3D.cpp:109-222,
R/Processor/Processor.cpp:567-600; mvs_gen_new_views, mvs_keypoint_cull).  Expected values come from the literal restatement
tests/ref_views.py; the scenarios are those tests/test_views_host.py checks from the restatement's diagnostics."""
import functools

import numpy as np
import pytest

from multiviewstitch_amd import _lib
from multiviewstitch_amd import scene as S
from tests import ref_views as RV
from tests.test_views_host import ALL_REMOVED_LIST, CVIEWS, EMPTY_LIST, SCENARIOS, cull_expected, cull_scenario, view_scenario


@pytest.fixture(scope="module")
def processor():
    from multiviewstitch_amd import processor
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return processor


def assert_same(got_views, got_tex, views, tex, tag):
    bad = np.flatnonzero(np.asarray(got_tex).reshape(-1) != np.asarray(tex).reshape(-1))
    assert len(bad) == 0, (tag, "tex", len(bad), bad[:8])
    bad = np.flatnonzero((np.asarray(got_views).reshape(-1, 3) != np.asarray(views).reshape(-1, 3)).any(1))
    assert len(bad) == 0, (tag, "pixels", len(bad), bad[:8])


# ------------------------------------------------------------------- 1. views ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_views_equal_the_restatement(processor, name):
    torch = pytest.importorskip("torch")
    cams, imgs, vc, axis, rot, (views, tex, _) = view_scenario(name)
    unpainted = tex == -1
    assert (views.reshape(tex.shape + (3,))[unpainted] == 0).all()                            # the restatement's own fill: (0,0,0) with tex = -1
    gv, gt = processor.GenNewViews(cams, imgs, vc, axis, rot)
    assert gv.dtype == np.uint8 and gt.dtype == np.int32 and gv.shape == views.shape and gt.shape == tex.shape
    assert_same(gv, gt, views, tex, (name, "host form"))
    dimg = torch.from_numpy(imgs).to("cuda")
    torch.cuda.synchronize()
    dv, dt = processor.GenNewViews(cams, dimg, vc, axis, rot, stream=torch.cuda.current_stream().cuda_stream)
    assert_same(dv.cpu().numpy(), dt.cpu().numpy(), views, tex, (name, "device form"))


@functools.lru_cache(maxsize=1)
def batch_inputs():
    q = cull_scenario()                                               # 3 frames, 3 cameras, 3 images at 96 x 72
    return q["cameras"], q["imgs"]


@pytest.mark.gpu
def test_a_batch_equals_one_frame_calls_and_the_stream_form_the_host_form(processor):
    torch = pytest.importorskip("torch")
    cams, imgs = batch_inputs()
    views, tex = processor.GenNewViews(cams, imgs, 4, 1, 7.5)
    assert not np.array_equal(views[0], views[1]) and not np.array_equal(tex[0], tex[2])
    for f in range(len(cams)):
        v1, t1 = processor.GenNewViews(cams[f:f + 1], imgs[f:f + 1], 4, 1, 7.5)
        assert_same(v1[0], t1[0], views[f], tex[f], ("frame", f))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dimg = torch.from_numpy(imgs).to("cuda", non_blocking=False)
        dv, dt = processor.GenNewViews(cams, dimg, 4, 1, 7.5, stream=side.cuda_stream)
    side.synchronize()
    assert_same(dv.cpu().numpy(), dt.cpu().numpy(), views, tex, "side stream")


@pytest.mark.gpu
def test_view_properties(processor):
    cams, imgs = batch_inputs()
    w, h = cams[0].w, cams[0].h
    views, tex = processor.GenNewViews(cams, imgs, 3, 0, 10.0)
    again = processor.GenNewViews(cams, imgs, 3, 0, 10.0)
    assert views.tobytes() == again[0].tobytes() and tex.tobytes() == again[1].tobytes()
    assert ((tex == -1) | ((tex >= 0) & (tex < w * h))).all()
    assert (views.reshape(len(cams), 3, w * h, 3)[tex == -1] == 0).all()
    assert 0.85 <= (tex != -1).mean() <= 1.0
    # the middle view (angle 0) takes the both-equal branch wherever uf and vf are integers: the pixel is the base pixel at tex
    branch = [RV.gen_view(cams[f], imgs[f], RV.homography(cams[f], 0, 0.0))[2]["branch_map"].reshape(-1) for f in range(len(cams))]
    seen = 0
    for f in range(len(cams)):
        px = np.flatnonzero(branch[f] == RV.BOTH_EQUAL)
        seen += len(px)
        assert np.array_equal(views[f, 1].reshape(-1, 3)[px], imgs[f].reshape(-1, 3)[tex[f, 1][px]])
    assert seen > 0


# -------------------------------------------------------------------- 2. cull ----
def assert_cull(r, what, keys_out, descs_out, with_descs):
    keep = np.concatenate([w == RV.SURVIVOR for w in what]).astype(np.uint8)
    off = np.zeros(len(keys_out) + 1, np.int64)
    off[1:] = np.cumsum([len(k) for k in keys_out])
    assert np.array_equal(np.asarray(r["keep"]), keep), np.flatnonzero(np.asarray(r["keep"]) != keep)[:8]
    assert np.array_equal(r["out_offsets"], off)
    assert np.asarray(r["keys"]).tobytes() == np.concatenate(keys_out).tobytes()
    if with_descs:
        assert np.asarray(r["descs"]).tobytes() == np.concatenate(descs_out).tobytes()
    else:
        assert r["descs"] is None


def flat_cull_args(q, with_descs, masked):
    off = np.zeros(len(q["keys"]) + 1, np.int64)
    off[1:] = np.cumsum([len(k) for k in q["keys"]])
    return (off, np.concatenate(q["keys"]), np.concatenate(q["descs"]) if with_descs else None, q["tex"], q["depths"]), (q["masks"] if masked else None)


@pytest.mark.gpu
@pytest.mark.parametrize("with_descs", (True, False))
@pytest.mark.parametrize("masked", (False, True))
def test_cull_equals_the_restatement(processor, with_descs, masked):
    q = cull_scenario()
    what, keys_out, descs_out = cull_expected(masked)
    (off, keys, descs, tex, depths), masks = flat_cull_args(q, with_descs, masked)
    r = processor.KeypointCull(q["cameras"], CVIEWS, off, keys, descs, tex, depths, S.MIN_DSP, S.MAX_DSP, masks)
    assert_cull(r, what, keys_out, descs_out, with_descs)
    gk, gd = processor.CullKeypoints(q["cameras"], q["depths"], q["tex"], q["keys"], q["descs"] if with_descs else None, S.MIN_DSP, S.MAX_DSP, masks)
    assert all(np.array_equal(a, b) for a, b in zip(gk, keys_out)) and len(gk) == len(keys_out)
    assert (gd is None) == (not with_descs)
    if with_descs:
        assert all(np.array_equal(a, b) for a, b in zip(gd, descs_out))


@pytest.mark.gpu
def test_cull_device_form_equals_the_restatement(processor):
    torch = pytest.importorskip("torch")
    q = cull_scenario()
    what, keys_out, descs_out = cull_expected(True)
    (off, keys, descs, tex, depths), masks = flat_cull_args(q, True, True)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (keys, descs, tex, depths, masks)]
    torch.cuda.synchronize()
    r = processor.KeypointCull(q["cameras"], CVIEWS, off, dev[0], dev[1], dev[2], dev[3], S.MIN_DSP, S.MAX_DSP, dev[4],
                               stream=torch.cuda.current_stream().cuda_stream)
    r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
    assert_cull(r, what, keys_out, descs_out, True)


@pytest.mark.gpu
def test_cull_scan_carries_past_its_first_chunk(processor):
    """The scan of the shared compaction tail takes 256 workgroup counts per turn and carries their sum into the next: more than
    65 536 + 256 keys give more than 257 workgroups of 256 keys, so the carry loop runs.  Every list of the scenario r times over;
    a key's fate does not depend on other keys, so the restatement's per-list results r times over are what is expected."""
    q = cull_scenario()
    what, keys_out, _ = cull_expected(True)
    n_keys = sum(len(k) for k in q["keys"])
    r = -(-(65536 + 256 + 1) // n_keys)
    keys = [np.tile(k, (r, 1)) for k in q["keys"]]
    total = sum(len(k) for k in keys)
    assert total > 65536 + 256 and (r - 1) * n_keys <= 65536 + 256
    (off, flat, _, tex, depths), masks = flat_cull_args(dict(q, keys=keys), False, True)
    got = processor.KeypointCull(q["cameras"], CVIEWS, off, flat, None, tex, depths, S.MIN_DSP, S.MAX_DSP, masks)
    assert_cull(got, [np.tile(w, r) for w in what], [np.tile(k, (r, 1)) for k in keys_out], None, False)
    oo = got["out_offsets"]
    assert off[EMPTY_LIST + 1] == off[EMPTY_LIST] and oo[EMPTY_LIST + 1] == oo[EMPTY_LIST]
    assert off[ALL_REMOVED_LIST + 1] > off[ALL_REMOVED_LIST] and oo[ALL_REMOVED_LIST + 1] == oo[ALL_REMOVED_LIST]


# --------------------------------------------------------------- 3. hand-over ----
def raw_for_tables(raw, tex1, tex2, w, h):
    """the generator's raw matches (made for its rolled identity tables: view 1 shifted right by one, view 2 up by one) re-expressed
    for real texIndex tables: the base pixel each one means, then a generated-view pixel of the same view that maps to it"""
    def base(a, gu, gv):
        return np.where(a == 1, (gu - 1) % w, gu), np.where(a == 2, (gv + 1) % h, gv)

    def inverse(tex):
        inv = np.full((tex.shape[0], w * h), -1, np.int64)
        for a in range(tex.shape[0]):
            g = np.flatnonzero(tex[a] >= 0)
            inv[a, tex[a][g]] = g
        return inv

    (u1, v1), (u2, v2) = base(raw[:, 0], raw[:, 1], raw[:, 2]), base(raw[:, 3], raw[:, 4], raw[:, 5])
    g1, g2 = inverse(tex1)[raw[:, 0], v1 * w + u1], inverse(tex2)[raw[:, 3], v2 * w + u2]
    ok = (g1 >= 0) & (g2 >= 0)
    return np.stack([raw[:, 0], g1 % w, g1 // w, raw[:, 3], g2 % w, g2 // w], 1)[ok].astype(np.int32)


@pytest.mark.gpu
def test_load_sequence_models_hands_over_to_the_chain(processor):
    from tests.test_gpu_match_pairs import SEQ_PRM, SH, SW, VIEWS, make_sequences
    seqs, _ = make_sequences([(0, 1), (2, 3)])
    models = [processor.LoadSequenceModels(q["cameras"], q["imgs"], q["depths"], VIEWS, 1, 4.0) for q in seqs]
    want = [RV.gen_new_views(q["cameras"], q["imgs"], VIEWS, 1, 4.0) for q in seqs]
    for m, q, (views, tex, _) in zip(models, seqs, want):
        assert set(m) == {"cameras", "depths", "tex", "imgs", "views"}
        assert_same(m["views"], m["tex"], views, tex, "sequence model")
    a, b = models
    a["raw"] = [[raw_for_tables(seqs[0]["raw"][i][j], a["tex"][i], b["tex"][j], SW, SH) for j in range(len(b["cameras"]))] for i in range(len(a["cameras"]))]
    assert min(len(r) for row in a["raw"] for r in row) > 100
    got = processor.CalcSimilarityTransformationSeq(models, dict(SEQ_PRM), 5)
    ref = [dict(cameras=q["cameras"], depths=q["depths"], tex=w[1], imgs=q["imgs"]) for q, w in zip(seqs, want)]
    ref[0]["raw"] = a["raw"]
    exp = processor.CalcSimilarityTransformationSeq(ref, dict(SEQ_PRM), 5)
    assert got[3] == exp[3] and all(np.array_equal(x, y) for x, y in zip(got[:3], exp[:3]))
    s, R, _ = seqs[0]["rel"]
    print("chain scale", got[0][0], "truth", s, "max |R - truth|", np.abs(got[1][0] - R).max())
