"""mvs_grid_mincut and mvs_grabcut_masks on the GPU (csrc/grabcut.hip).  The cut is held to scipy's maximum flow byte for byte (rule G1
makes the answer unique, so every case is an equality); the segmentation is held to the restatement tests/ref_grabcut.py link by link
through mvs_test_grabcut_trace: every step is compared from the DEVICE's previous step, so no drift can accumulate."""
import ctypes as C
import functools

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import grabcut_scenes as SC, ref_grabcut as R

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the cut ----
def _random_case(seed, gw, gh, emax=4000, cmax=300):
    rng = np.random.default_rng(seed)
    e = rng.integers(-emax, emax + 1, (gh, gw)).astype(np.int32)
    cap = rng.integers(0, cmax + 1, (8, gh, gw)).astype(np.int32)             # asymmetric; entries that leave the grid stay: ignored
    cap[rng.random(cap.shape) < 0.3] = 0
    return e, cap


def _serpentine(gw=31, gh=21):
    """a corridor one node wide that runs along every second row, joined at alternating ends: source excess at one end, the sink at
    the other, capacity along the corridor only.  Its breadth-first depth is its length, far above gw + gh."""
    open_ = np.zeros((gh, gw), bool)
    open_[0::2] = True
    for k, y in enumerate(range(1, gh, 2)):
        open_[y, gw - 1 if k % 2 == 0 else 0] = True
    cap = np.zeros((8, gh, gw), np.int32)
    for d in (0, 2, 4, 6):
        ok, nb = R.neighbour(gw, gh, d)
        cap[d] = np.where(ok & open_ & open_.reshape(-1)[nb], 7, 0)
    cap[4][gh // 2 // 2 * 2][gw // 2] = cap[0][gh // 2 // 2 * 2][gw // 2 + 1] = 3      # a bottleneck half way: what lies before it ends on the source side
    e = np.zeros((gh, gw), np.int32)
    e[0, 0] = 5
    last = (gh - 1 if (gh - 1) % 2 == 0 else gh - 2)
    e[last, gw - 1 if ((last // 2) % 2 == 0) else 0] = -9
    assert int(open_.sum()) > 4 * (gw + gh)
    return e, cap


@functools.lru_cache(maxsize=None)
def _cases():
    out = {}
    out["random 40x30"] = _random_case(11, 40, 30)
    out["random 67x35"] = _random_case(12, 67, 35)
    out["serpentine"] = _serpentine()
    out["equal capacities"] = SC.equal_caps()
    e, cap = _random_case(13, 20, 17)
    out["zero capacities"] = (e, np.zeros_like(cap))
    e, cap = _random_case(14, 24, 18)
    e = np.abs(e)
    e[:, 12:] = 0                                                            # excess, and no sink anywhere
    out["no sink"] = (e, cap)
    e, cap = _random_case(15, 33, 20)
    cap[:, :, 16] = 0                                                        # ... and a sink the excess cannot reach: column 16 is a wall
    for d in range(8):
        ok, nb = R.neighbour(33, 20, d)
        cap[d][(nb % 33 == 16) & ok] = 0
    e[:, :16] = np.abs(e[:, :16])
    out["unreachable sink"] = (e, cap)
    out["1x1 source"] = (np.array([[5]], np.int32), np.full((8, 1, 1), 9, np.int32))
    out["1x1 sink"] = (np.array([[-5]], np.int32), np.full((8, 1, 1), 9, np.int32))
    out["1x1 zero"] = (np.array([[0]], np.int32), np.full((8, 1, 1), 9, np.int32))
    out["1xN"] = _random_case(16, 37, 1)
    out["Nx1"] = _random_case(17, 1, 37)
    for e, cap in out.values():
        e.setflags(write=False)
        cap.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(name):
    e, cap = _cases()[name]
    return R.g1_cut(e, cap)


@pytest.mark.parametrize("name", ["random 40x30", "random 67x35", "serpentine", "equal capacities", "zero capacities", "no sink",
                                  "unreachable sink", "1x1 source", "1x1 sink", "1x1 zero", "1xN", "Nx1"])
def test_mincut_equals_scipy(name):
    e, cap = _cases()[name]
    side, rounds = P.GridMinCut(e[None], cap[None], with_rounds=True)
    print(f"{name}: rounds = {rounds}, source side = {int(side.sum())} of {side.size}")
    assert np.array_equal(side[0], _expected(name))


def test_mincut_batch_of_unequal_difficulty_and_two_runs():
    """a 31 x 21 batch: the serpentine next to an all-zero grid and a random one; and the same bytes twice"""
    es, caps = _serpentine()
    er, capr = _random_case(21, 31, 21)
    e = np.stack([es, np.zeros_like(es), er])
    cap = np.stack([caps, np.zeros_like(caps), capr])
    a = P.GridMinCut(e, cap)
    b = P.GridMinCut(e, cap)
    assert np.array_equal(a, b)
    for g in range(3):
        assert np.array_equal(a[g], R.g1_cut(e[g], cap[g])), g


def test_mincut_device_form_on_a_stream():
    import torch
    e, cap = _cases()["random 67x35"]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        de, dc = torch.from_numpy(e[None].copy()).cuda(), torch.from_numpy(cap[None].copy()).cuda()
        side = P.GridMinCut(de, dc, stream=st.cuda_stream)
    st.synchronize()
    assert side.is_cuda and np.array_equal(side.cpu().numpy()[0], _expected("random 67x35"))


def test_mincut_round_cap_is_an_error_and_the_process_goes_on():
    """max_rounds = 1 on the serpentine: one round of relabelling cannot cross the corridor"""
    e, cap = _cases()["serpentine"]
    with pytest.raises(L.MvsError) as err:
        P.GridMinCut(e[None], cap[None], max_rounds=1)
    assert err.value.code == -7 and "max_rounds" in str(err.value)
    assert np.array_equal(P.GridMinCut(e[None], cap[None])[0], _expected("serpentine"))


def test_mincut_headroom_is_checked_on_the_device_form():
    import torch
    e = torch.full((1, 4, 4), 2 ** 30, dtype=torch.int32, device="cuda")
    cap = torch.full((1, 8, 4, 4), 2 ** 28, dtype=torch.int32, device="cuda")
    with pytest.raises(L.MvsError) as err:
        P.GridMinCut(e, cap)
    assert err.value.code == -1


# ---------------------------------------------------------------- the segmentation ----
@functools.lru_cache(maxsize=None)
def _trace(name):
    imgs, _, p = SC.scene(name)
    n, h, w = imgs.shape[:3]
    N, it = (w // 2) * (h // 2), p["iters"]
    prm = P.grabcut_params(**p)
    t = dict(mask=np.zeros((n, h, w), np.uint8), S=np.zeros(n, np.int64), ncap=np.zeros((n, 8, h // 2, w // 2), np.int32),
             labels=np.zeros((it + 1, n, h // 2, w // 2), np.uint8), sums=np.zeros((it + 1, n, 2, 5, 10), np.int64),
             excess=np.zeros((it, n, h // 2, w // 2), np.int32), half_mask=np.zeros((it, n, h // 2, w // 2), np.uint8), rounds=np.zeros(it, np.int32))
    assert t["labels"].size == (it + 1) * n * N
    img = np.ascontiguousarray(imgs)
    L.check(L.lib().mvs_test_grabcut_trace(n, w, h, L.ptr(img), C.byref(prm), *[L.ptr(t[k]) for k in
                                           ("mask", "S", "ncap", "labels", "sums", "excess", "half_mask", "rounds")]))
    print(f"{name}: rounds per cut = {t['rounds'].tolist()}")
    for a in t.values():
        a.setflags(write=False)
    return t


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_grabcut_trace_link_by_link(name):
    imgs, _, p = SC.scene(name)
    ref = SC.reference(name)
    t = _trace(name)
    n, h, w = imgs.shape[:3]
    for f in range(n):
        r = ref[f]
        half, inside = r["half"], r["inside"]
        assert int(t["S"][f]) == r["S"]                                                        # beta's sum: exact
        assert np.abs(t["ncap"][f].astype(np.int64) - r["cap"]).max() <= 1                      # one unit: exp's last bit across llrint
        assert np.array_equal(t["ncap"][f], np.stack([t["ncap"][f][d ^ 4].reshape(-1)[R.neighbour(w // 2, h // 2, d)[1]].reshape(h // 2, w // 2) *
                                                      R.neighbour(w // 2, h // 2, d)[0] for d in range(8)]))   # symmetric
        assert np.array_equal(t["labels"][0][f], r["labels0"])                                  # rule 4: integers
        assert np.array_equal(t["sums"][0][f], R.learn_sums(half, inside, t["labels"][0][f]))
        fg, models = inside, R.fit_models(t["sums"][0][f])
        for i in range(p["iters"]):
            lab, gap = R.assign(models, half, fg)
            dev_lab = t["labels"][i + 1][f]
            assert np.array_equal(dev_lab[gap >= 1e-9], lab[gap >= 1e-9])                       # the argmax, from the device's own mask
            assert np.array_equal(t["sums"][i + 1][f], R.learn_sums(half, fg, dev_lab))        # the sums on the device's labels: exact
            models = R.fit_models(t["sums"][i + 1][f])
            e, _ = R.excess_of(models, half, inside, p["gamma"])
            assert np.abs(t["excess"][i][f].astype(np.int64) - e).max() <= 1
            cut = R.g1_cut(t["excess"][i][f], t["ncap"][f])                                     # G1 of the device's own links: exact
            fg = inside & (cut != 0)
            assert np.array_equal(t["half_mask"][i][f] != 0, fg)
        assert np.array_equal(t["mask"][f], R.full_mask(t["half_mask"][-1][f], w, h))           # rule 12: exact


def test_grabcut_public_forms_agree_with_the_trace():
    import torch
    imgs, truth, p = SC.scene("s1")
    t = _trace("s1")
    prm = P.grabcut_params(**p)
    mask, half = P.GrabCutMasks(np.ascontiguousarray(imgs), prm, with_half=True)
    assert np.array_equal(mask, t["mask"]) and np.array_equal(half, t["half_mask"][-1])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dm = P.GrabCutMasks(torch.from_numpy(imgs.copy()).cuda(), prm, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(dm.cpu().numpy(), mask)
    assert set(np.unique(mask)) <= {0, 255}
    for f in range(len(imgs)):
        assert SC.iou(half[f], SC.half_truth(truth[f])) >= 0.9
        assert SC.iou(mask[f], truth[f]) >= SC.FULL_IOU_FLOOR


def test_grabcut_cut_that_needs_more_rounds_is_an_error():
    imgs, _, p = SC.scene("s1")
    with pytest.raises(L.MvsError) as err:
        P.GrabCutMasks(np.ascontiguousarray(imgs), P.grabcut_params(max_rounds=1, **p))
    assert err.value.code == -7


# ---------------------------------------------------------------- the chain ----
def test_load_sequence_models_with_segment():
    """LoadSequenceModels(segment=...) drops exactly the keys CullKeypoints drops when handed the same masks, and segment=None is
    today's result"""
    from multiviewstitch_amd import scene as S
    from tests import sift_scenes as SS
    from tests.test_views_host import CFRAMES, CH, CVIEWS, CW
    cams, depths = S.make_sequence(CFRAMES, CW, CH, 25.0, f=2.2)
    imgs = np.stack([SS.scene(CW, CH, 40 + i) for i in range(CFRAMES)])
    seg = P.grabcut_params(hl=0.15, hr=0.15, vl=0.15, vr=0.15)
    kw = dict(view_count=CVIEWS, axis=0, rot_angle=10.0, sift=P.sift_params(hl=0.05, vr=0.05), min_dsp=S.MIN_DSP, max_dsp=S.MAX_DSP)
    plain = P.LoadSequenceModels(cams, imgs, depths, **kw)
    again = P.LoadSequenceModels(cams, imgs, depths, segment=None, **kw)
    assert "masks" not in again
    for a, b in zip(plain["keys"] + plain["descs"], again["keys"] + again["descs"]):
        assert a.tobytes() == b.tobytes()
    seg_out = P.LoadSequenceModels(cams, imgs, depths, segment=seg, **kw)
    masks = P.GrabCutMasks(imgs, seg)
    assert np.array_equal(seg_out["masks"], masks)
    by_hand = P.LoadSequenceModels(cams, imgs, depths, masks=masks, **kw)
    for a, b in zip(seg_out["keys"] + seg_out["descs"], by_hand["keys"] + by_hand["descs"]):
        assert a.tobytes() == b.tobytes()
    assert sum(len(k) for k in seg_out["keys"]) <= sum(len(k) for k in plain["keys"])
