"""mvs_draw_overlays, mvs_match_overlays, mvs_sift_overlays and their file forms on the GPU (csrc/overlay.hip) against the restatement
tests/ref_overlay.py, byte for byte: the cases of tests/test_overlay_host.py (ragged tiles, every kind at the corners and clipped, every
slope and thickness, 300 overlapping primitives across the chunk boundary, the widest canvas with the thickest line), 70 canvases in one
call, the device form in place on a stream, the stacked match canvases with one generator through the pairs, the SIFT marks at the
rounding ties, and the files in one batch and in three."""
import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import ref_overlay as R
from tests.test_overlay_host import cases, want

pytestmark = pytest.mark.gpu
CASES = {what: (canvas, prims) for what, canvas, prims in cases()}
SMALL = [what for what, (canvas, _) in CASES.items() if canvas.shape[:2] == (29, 37)]


def test_every_small_case_alone_and_all_in_one_call():
    """n = 1, and all 37 x 29 cases as the canvases of one call"""
    assert len(SMALL) >= 18
    for what in SMALL:
        canvas, prims = CASES[what]
        got = P.DrawOverlays(canvas[None], [prims])
        assert got.shape == (1, 29, 37, 3) and np.array_equal(got[0], want(what, canvas, prims)), what
    got = P.DrawOverlays(np.stack([CASES[w][0] for w in SMALL]), [CASES[w][1] for w in SMALL])
    for i, what in enumerate(SMALL):
        assert np.array_equal(got[i], want(what, *CASES[what])), what


def test_order_across_the_chunk_boundary():
    """300 primitives are more than one chunk of 256: with a canvas-covering disc last every tile exits after its first chunk, with it
    first everything paints over it and the second chunk is read to the end"""
    canvas, many = CASES["order_300"]
    assert len(many) == 300 and len({p[6] for p in many}) == 300
    last = P.DrawOverlays(canvas[None], [CASES["order_cover_last"][1]])[0]
    assert (last == np.array([1, 2, 3], np.uint8)).all()
    first = P.DrawOverlays(canvas[None], [CASES["order_cover_first"][1]])[0]
    assert np.array_equal(first, want("order_cover_first", *CASES["order_cover_first"]))
    plain = want("order_300", canvas, many)
    untouched = (plain == canvas).all(axis=2)
    assert (first[untouched] == np.array([1, 2, 3], np.uint8)).all() and np.array_equal(first[~untouched], plain[~untouched])
    low = R.draw(canvas, many[:44])                                  # the pixels the second chunk (indices 43 .. 0) decides
    decided = (plain == low).all(axis=2) & ~untouched
    print("pixels decided by the second chunk:", int(decided.sum()), "untouched:", int(untouched.sum()))
    assert decided.sum() >= 10
    assert np.array_equal(P.DrawOverlays(canvas[None], [many])[0][decided], plain[decided])


def test_70_canvases_with_lists_of_different_lengths():
    rng = np.random.default_rng(70)
    many = CASES["order_300"][1]
    imgs = rng.integers(0, 256, (70, 29, 37, 3), dtype=np.uint8)
    lists = [[] if i % 5 == 0 else many[(3 * i) % 40:(3 * i) % 40 + (37 * i) % 290] for i in range(70)]
    assert max(len(p) for p in lists) > 256 and sum(not p for p in lists) == 14
    got = P.DrawOverlays(imgs, lists)
    for i in range(70):
        assert np.array_equal(got[i], R.draw(imgs[i], lists[i])), i
        if not lists[i]:
            assert np.array_equal(got[i], imgs[i])


def test_the_widest_canvas_with_the_thickest_line():
    """16384 x 8, (0, 0) - (16383, 7) at T = 255: the largest products of O3, against Python integers.  That line covers all eight
    rows; the same line at T = 3 leaves pixels of every tile to the source"""
    canvas, prims = CASES["wide_T255"]
    got = P.DrawOverlays(canvas[None], [prims])[0]
    assert np.array_equal(got, want("wide_T255", canvas, prims)) and (got == np.array([9, 8, 7], np.uint8)).all()
    canvas, prims = CASES["wide_T3"]
    got = P.DrawOverlays(canvas[None], [prims])[0]
    w = want("wide_T3", canvas, prims)
    assert np.array_equal(got, w) and (w == canvas).all(axis=2).any() and (w != canvas).any()
    canvas, prims = CASES["diagonal_512"]
    assert np.array_equal(P.DrawOverlays(canvas[None], [prims])[0], want("diagonal_512", canvas, prims))


def test_the_device_form_in_place_on_a_stream_and_two_runs():
    import torch
    names = ["order_300", "segments_T3", "kind1_outside", "empty"]
    imgs = np.stack([CASES[w][0] for w in names])
    lists = [CASES[w][1] for w in names]
    host = P.DrawOverlays(imgs, lists)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.as_tensor(imgs).to("cuda")
    a = P.DrawOverlays(t, lists, stream=s.cuda_stream)
    assert a.is_cuda and a.data_ptr() != t.data_ptr() and np.array_equal(t.cpu().numpy(), imgs)
    b = P.DrawOverlays(t, lists, stream=s.cuda_stream)
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), host)          # two runs give the same bytes
    c = P.DrawOverlays(t, lists, stream=s.cuda_stream, in_place=True)            # out == in
    assert c.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), host)
    assert np.array_equal(P.DrawOverlays(imgs, lists, device="cuda").cpu().numpy(), host)


def _match_inputs():
    rng = np.random.default_rng(32)
    n1, n2, w, h = 3, 2, 40, 24
    imgs1 = rng.integers(0, 256, (n1, h, w, 3), dtype=np.uint8)
    imgs2 = rng.integers(0, 256, (n2, h, w, 3), dtype=np.uint8)
    counts = [[5, 0], [9, 3], [1, 12]]                                # pair (0, 1) has no match
    matches = [[np.stack([rng.integers(0, w, c), rng.integers(0, h, c), rng.integers(0, w, c), rng.integers(0, h, c)], axis=1).astype(np.int32)
                for c in row] for row in counts]
    matches[1][0][0] = (0, 0, w - 1, h - 1)                           # the corners of the stack
    matches[1][0][1] = (w - 1, h - 1, 0, 0)                           # the two rows where the sources meet
    return imgs1, imgs2, matches, sum(sum(row) for row in counts)


def test_match_overlays():
    import torch
    imgs1, imgs2, matches, total = _match_inputs()
    h = 24
    st = np.array([R.RNG_DEFAULT], np.uint64)
    got = P.MatchOverlays(imgs1, imgs2, matches, rng_state=st)
    ref, state = R.match_canvases(imgs1, imgs2, matches)
    assert got.shape == (6, 48, 40, 3) and np.array_equal(got, ref)
    g = R.Rng()
    for _ in range(6 * total):
        g.next()
    assert int(st[0]) == state == g.state                             # 6 draws per match
    assert np.array_equal(got[1], np.concatenate([imgs1[0], imgs2[1]], axis=0))      # no match: the plain stack
    # rows h - 1 and h come from imgs1[i] and imgs2[j]: pair (0, 0) has 5 lines of at most 3 pixels a row, the rest of a row is the source's
    assert (got[0][h - 1] == imgs1[0][h - 1]).all(axis=1).sum() >= 20 and (got[0][h] == imgs2[0][0]).all(axis=1).sum() >= 20
    assert (got[5][h - 1] == imgs1[2][h - 1]).all(axis=1).sum() >= 4 and (got[5][h] == imgs2[1][0]).all(axis=1).sum() >= 4
    assert np.array_equal(P.MatchOverlays(imgs1, imgs2, matches), ref)                # NULL: a fresh default generator
    colours = [tuple(p[6]) for p in R.match_prims(np.concatenate([m for row in matches for m in row]), h, R.Rng())[2::3]]
    assert [tuple(c) for c in P.cv_rng_colours(total)[0].tolist()] == colours and len(set(colours)) == total
    st2 = np.array([R.RNG_DEFAULT], np.uint64)
    t = P.MatchOverlays(torch.as_tensor(imgs1).to("cuda"), torch.as_tensor(imgs2).to("cuda"), matches, rng_state=st2)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), ref) and int(st2[0]) == state
    carried, state2 = R.match_canvases(imgs1, imgs2, matches, state)
    assert np.array_equal(P.MatchOverlays(imgs1, imgs2, matches, rng_state=st), carried) and int(st[0]) == state2
    assert not np.array_equal(carried, ref)


def test_sift_overlays():
    import torch
    rng = np.random.default_rng(33)
    w, h = 37, 29
    views = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    keys = [np.array([[2.5, 5.0, 1.0, 0.0], [3.5, 11.0, 1.0, 0.0], [w - 0.4, 20.0, 1.0, 0.0], [np.nan, 7.0, 1.0, 0.0], [9.0, np.nan, 1.0, 0.0],
                      [-0.5, 0.5, 2.0, 0.1], [np.inf, 3.0, 1.0, 0.0], [12.5, 28.5, 1.0, 0.0], [1e12, -1e12, 1.0, 0.0]], np.float32),
            np.zeros((0, 4), np.float32),
            (rng.random((400, 4)) * [w + 4, h + 4, 1, 1] - [2, 2, 0, 0]).astype(np.float32)]
    got = P.SiftOverlays(views, keys)
    assert np.array_equal(got, R.sift_canvases(views, keys)) and np.array_equal(got[1], views[1])
    green = (got[0] == np.array([0, 255, 0], np.uint8)).all(axis=2) & ~(views[0] == np.array([0, 255, 0], np.uint8)).all(axis=2)
    plus = lambda x, y: {(x, y), (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)}
    expect = plus(2, 5) | plus(4, 11) | {(w - 1, 20)} | plus(0, 0) | plus(12, 28)       # 2.5 -> 2, 3.5 -> 4, w - 0.4 -> w: a clipped plus
    expect = {(x, y) for x, y in expect if 0 <= x < w and 0 <= y < h}
    assert {(x, y) for y, x in zip(*np.nonzero(green))} == expect
    t = torch.as_tensor(views).to("cuda")
    assert np.array_equal(P.SiftOverlays(t, keys).cpu().numpy(), got)
    P.SiftOverlays(t, keys, in_place=True)
    assert np.array_equal(t.cpu().numpy(), got)


def test_the_match_files(tmp_path, monkeypatch):
    imgs1, imgs2, matches, _ = _match_inputs()
    ref, state = R.match_canvases(imgs1, imgs2, matches)
    streams = P.EncodeJpegs(ref)
    names = sorted(f"match4_{i}_{j}.jpg" for i in range(3) for j in range(2))
    st = np.array([R.RNG_DEFAULT], np.uint64)
    P.MatchOverlayFiles(str(tmp_path / "a" / "Match"), 4, imgs1, imgs2, matches, rng_state=st)      # without the trailing '/'
    assert int(st[0]) == state and sorted(p.name for p in (tmp_path / "a" / "Match").iterdir()) == names
    monkeypatch.setenv("MVS_OVERLAY_BATCH_BYTES", str(2 * ref[0].size))                            # two canvases per batch: three batches
    P.MatchOverlayFiles(str(tmp_path / "b") + "/", 4, imgs1, imgs2, matches)
    monkeypatch.setenv("MVS_OVERLAY_BATCH_BYTES", "1")                                             # below one canvas: one per batch
    P.MatchOverlayFiles(str(tmp_path / "c"), 4, imgs1, imgs2, matches)
    monkeypatch.delenv("MVS_OVERLAY_BATCH_BYTES")
    P.MatchOverlayFiles(str(tmp_path / "d"), 4, np.ascontiguousarray(imgs1[..., ::-1]), np.ascontiguousarray(imgs2[..., ::-1]), matches, order="RGB")
    for d in ("a/Match", "b", "c", "d"):
        assert sorted(p.name for p in (tmp_path / d).iterdir()) == names, d
        for i in range(3):
            for j in range(2):
                assert (tmp_path / d / f"match4_{i}_{j}.jpg").read_bytes() == streams[2 * i + j], (d, i, j)
    swapped, _ = R.match_canvases(imgs1[..., ::-1], imgs2[..., ::-1], matches, swap=True)
    assert np.array_equal(swapped[..., ::-1], ref)                    # the restatement's own swap: the same picture
    P.MatchOverlayFiles(str(tmp_path / "q"), 0, imgs1, imgs2, matches, quality=60, sampling="444", restart_interval=3)
    assert (tmp_path / "q" / "match0_2_1.jpg").read_bytes() == P.EncodeJpegs(ref[5:], quality=60, sampling="444", restart_interval=3)[0]


def test_the_sift_files(tmp_path, monkeypatch):
    rng = np.random.default_rng(34)
    w, h = 37, 29
    views = rng.integers(0, 256, (3, 2, h, w, 3), dtype=np.uint8)
    keys = [(rng.random((n, 4)) * [w + 2, h + 2, 1, 1] - [1, 1, 0, 0]).astype(np.float32) for n in (30, 0, 7, 120, 1, 55)]
    streams = P.EncodeJpegs(R.sift_canvases(views.reshape(6, h, w, 3), keys))
    names = sorted(f"proj{i}_{j}.jpg" for i in range(3) for j in range(2))
    P.SiftOverlayFiles(str(tmp_path / "s"), "Sift", views, keys)
    monkeypatch.setenv("MVS_OVERLAY_BATCH_BYTES", str(2 * h * w * 3))                              # three batches
    P.SiftOverlayFiles(str(tmp_path / "s") + "/", "Sift1", views, keys)
    monkeypatch.delenv("MVS_OVERLAY_BATCH_BYTES")
    assert sorted(p.name for p in (tmp_path / "s" / "Views").iterdir()) == ["Sift", "Sift1"]
    for sub in ("Sift", "Sift1"):
        assert sorted(p.name for p in (tmp_path / "s" / "Views" / sub).iterdir()) == names
        for i in range(3):
            for j in range(2):
                assert (tmp_path / "s" / "Views" / sub / f"proj{i}_{j}.jpg").read_bytes() == streams[2 * i + j], (sub, i, j)


def test_the_chain_writes_the_match_pictures(tmp_path):
    """CalcSimilarityTransformationSeq(match_dir=...): the same chain as without, and pair k's files are the pictures of the lists
    MatchFilterPairs returns for that pair's inputs"""
    from tests.test_gpu_match_pairs import SEQ_PRM, chain_scenario
    seqs = chain_scenario()[0]
    plain = P.CalcSimilarityTransformationSeq(seqs, dict(SEQ_PRM), 5)
    got = P.CalcSimilarityTransformationSeq(seqs, dict(SEQ_PRM), 5, match_dir=tmp_path / "Match")
    for a, b in zip(plain[:3], got[:3]):
        assert np.array_equal(a, b)
    assert plain[3] == got[3]
    n = 0
    for k in range(2):
        a, b = seqs[k], seqs[k + 1]
        valid = [np.asarray(q["valid"], np.uint8).reshape(len(q["imgs"]), -1) for q in (a, b)]
        matches, _ = P.MatchFilterPairs(a["raw"], a["tex"], valid[0], b["tex"], valid[1], a["imgs"], b["imgs"], SEQ_PRM["ssd_win"], SEQ_PRM["ssd_err"],
                                        SEQ_PRM["sample_interval"])
        streams = P.EncodeJpegs(P.MatchOverlays(a["imgs"], b["imgs"], matches))              # one fresh generator per sequence pair
        n2 = len(b["imgs"])
        for i in range(len(a["imgs"])):
            for j in range(n2):
                assert (tmp_path / "Match" / f"match{k}_{i}_{j}.jpg").read_bytes() == streams[i * n2 + j], (k, i, j)
                n += 1
        assert sum(len(m) for row in matches for m in row) > 100
    assert len(list((tmp_path / "Match").iterdir())) == n == 8
