"""The loop over adjacent sequences of Processor::CalcSimilarityTransformationSeq on the GPU (R/Processor/Processor.cpp:629-826):
the batched match-filter cascade (mvs_match_filter_pairs), one sequence pair end to end (mvs_sequence_pair_srt) and the chain
(processor.CalcSimilarityTransformationSeq).  Every expected value is built from the oracle's one-pair functions in the test."""
import functools
import math

import numpy as np
import pytest

from multiviewstitch_amd import _lib
from multiviewstitch_amd import io as mio
from multiviewstitch_amd import scene as S
from oracle import binding as O
from tests.test_match_filter import scene

W, H, VIEWS, WIN = 96, 72, 3, 3                                     # the generator's shape

SETTINGS = ((6.0, 5), (12.0, 0), (3.0, 9))
N1, N2 = 3, 2
PLAIN, EMPTY, OUTSIDE, REPEATED, LARGE = (0, 3), 1, 2, 4, 5          # what bucket k = i * N2 + j holds


@pytest.fixture(scope="module")
def processor():
    from multiviewstitch_amd import processor
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return processor


# ------------------------------------------------------------------ 1. cascade ----
@functools.lru_cache(maxsize=1)
def cascade_inputs():
    """3 x 2 frame pairs at 96 x 72: every frame has its own image, tex stack and mask (tests/test_match_filter.py's generator with
    a seed per frame); the buckets are two plain ones, an empty one, one of out-of-range pixels only, one match repeated 50 times
    and one of 16 000 random matches."""
    f1 = [scene(10 + i) for i in range(N1)]
    f2 = [scene(20 + j) for j in range(N2)]
    tex1, valid1, imgs1 = (np.stack([f[c] for f in f1]) for c in (1, 2, 5))
    tex2, valid2, imgs2 = (np.stack([f[c] for f in f2]) for c in (3, 4, 6))
    rng = np.random.default_rng(3)
    raw = {k: scene(100 + k)[0] for k in PLAIN}
    raw[EMPTY] = np.empty((0, 6), np.int32)
    out = rng.integers(0, VIEWS, (40, 6))
    out[:, 1], out[:, 2] = rng.choice([-3, -1, W, W + 5], 40), rng.integers(0, H, 40)
    out[:, 4], out[:, 5] = rng.integers(0, W, 40), rng.choice([-1, H, H + 2], 40)
    raw[OUTSIDE] = out.astype(np.int32)
    i, j = divmod(REPEATED, N2)
    ok = np.flatnonzero((tex1[i, 0] != -1) & valid1[i].astype(bool) & (np.roll(tex2[j, 0], -4) != -1) & np.roll(valid2[j], -4).astype(bool))
    px = int(ok[(ok % W > 10) & (ok % W < W - 14) & (ok // W > 10) & (ok // W < H - 10)][0])
    raw[REPEATED] = np.tile(np.array([0, px % W, px // W, 0, px % W + 4, px // W], np.int32), (50, 1))
    big = np.stack([rng.integers(0, VIEWS, 16000), rng.integers(0, W, 16000), rng.integers(0, H, 16000),
                    rng.integers(0, VIEWS, 16000), rng.integers(0, W, 16000), rng.integers(0, H, 16000)], 1).astype(np.int32)
    raw[LARGE] = big
    raw = [[raw[i * N2 + j] for j in range(N2)] for i in range(N1)]
    return raw, tex1, valid1, tex2, valid2, imgs1, imgs2


@functools.lru_cache(maxsize=None)
def cascade_expected(win, ssd_err, interval):
    raw, tex1, valid1, tex2, valid2, imgs1, imgs2 = cascade_inputs()
    return [[O.match_filter(raw[i][j], tex1[i], valid1[i], tex2[j], valid2[j], imgs1[i], imgs2[j], win, ssd_err, interval) for j in range(N2)]
            for i in range(N1)]


def assert_cascade(got, cnt, want):
    for i in range(N1):
        for j in range(N2):
            assert np.array_equal(cnt[i, j], want[i][j][1]), (i, j, cnt[i, j], want[i][j][1])
            assert np.array_equal(got[i][j], want[i][j][0]), (i, j)


def test_the_cascade_scenario_holds_what_it_should():
    for ssd_err, interval in SETTINGS:
        want = cascade_expected(WIN, ssd_err, interval)
        cnt = {i * N2 + j: tuple(want[i][j][1]) for i in range(N1) for j in range(N2)}
        for k in PLAIN:
            print("plain bucket", k, (ssd_err, interval), cnt[k])
            assert cnt[k][0] > cnt[k][1] > cnt[k][2] > 10, (k, ssd_err, interval, cnt[k])
        assert cnt[EMPTY] == (0, 0, 0) and cnt[OUTSIDE] == (0, 0, 0)
        assert cnt[REPEATED][0] == 1 and cnt[REPEATED][1] in (0, 1) and cnt[REPEATED][2] == cnt[REPEATED][1]
        assert cnt[LARGE][0] > 8192


@pytest.mark.gpu
@pytest.mark.parametrize("ssd_err,interval", SETTINGS)
def test_cascade_parity(processor, monkeypatch, ssd_err, interval):
    args = cascade_inputs()
    want = cascade_expected(WIN, ssd_err, interval)
    got, cnt = processor.MatchFilterPairs(*args, WIN, ssd_err, interval)
    assert_cascade(got, cnt, want)
    monkeypatch.setenv("MVS_MATCH_PAIRS_LDS_CAP", "256")             # the plain 900-match buckets through the workspace path too
    got, cnt = processor.MatchFilterPairs(*args, WIN, ssd_err, interval)
    assert_cascade(got, cnt, want)


@pytest.mark.gpu
def test_cascade_without_a_window(processor):
    got, cnt = processor.MatchFilterPairs(*cascade_inputs(), 0, 6.0, 5)
    assert_cascade(got, cnt, cascade_expected(0, 6.0, 5))


@pytest.mark.gpu
def test_cascade_rejects_a_view_index_out_of_range(processor):
    raw, *rest = cascade_inputs()
    bad = [[r.copy() for r in row] for row in raw]
    bad[1][1][7, 0] = VIEWS                                          # view1 = view_count
    with pytest.raises(_lib.MvsError) as e:
        processor.MatchFilterPairs(bad, *rest, WIN, 6.0, 5)
    assert e.value.code == -1


@pytest.mark.gpu
def test_cascade_dev_form_equals_the_host_form(processor):
    torch = pytest.importorskip("torch")
    raw, *stacks = cascade_inputs()
    dev = [torch.from_numpy(a).to("cuda") for a in stacks]
    torch.cuda.synchronize()
    got, cnt = processor.MatchFilterPairs(raw, *dev, WIN, 6.0, 5, stream=torch.cuda.current_stream().cuda_stream)
    assert_cascade(got, cnt, cascade_expected(WIN, 6.0, 5))
    host, hcnt = processor.MatchFilterPairs(raw, *stacks, WIN, 6.0, 5)
    assert np.array_equal(cnt, hcnt) and all(np.array_equal(got[i][j], host[i][j]) for i in range(N1) for j in range(N2))


# ------------------------------------------------------------ 2. sequence pair ----
SW, SH = 160, 120
SEQ_PRM = dict(ssd_win=2, ssd_err=1e6, sample_interval=2, min_dsp=S.MIN_DSP, max_dsp=S.MAX_DSP, min_match_count=7, ransac_iters=200,
               pixel_err=6.0, adapt_ratio=0.75)


def similarity(k):
    """q = s R p + t of sequence k's frame of reference (sequence 0: the frame the surface was made in)"""
    if k == 0:
        return 1.0, np.eye(3), np.zeros(3)
    rng = np.random.default_rng(40 + k)
    return (1.15, 0.9)[k % 2 == 0], S._rot_axis(rng.normal(size=3), math.radians(20.0)), rng.uniform(-0.1, 0.1, 3)


def in_frame(cam, depth, s, R, t):
    """the camera and raster of a frame after the world is re-expressed as q = s R p + t (tests/test_pipeline.py's world camera)"""
    Rc = np.asarray(cam.R)
    return S.Camera(cam.fx, cam.fy, cam.cx, cam.cy, Rc @ R.T, s * np.asarray(cam.t) - Rc @ R.T @ t, cam.w, cam.h), (depth.astype(np.float64) / s).astype(np.float32)


def tex_tables():
    idx = np.arange(SW * SH, dtype=np.int32).reshape(SH, SW)
    return np.stack([idx, np.roll(idx, 1, axis=1), np.roll(idx, -1, axis=0)]).reshape(VIEWS, -1)


def image(cam_index, rng):
    yy, xx = np.mgrid[0:SH, 0:SW]
    base = 128 + 60 * np.sin(xx / 9.0 + cam_index) * np.cos(yy / 7.0)
    return np.clip(np.stack([base, 0.8 * base + 20, 255 - base], -1) + rng.normal(scale=2, size=(SH, SW, 3)), 0, 255).astype(np.uint8)


def raw_matches(rng, pts_i, valid_i, rel, cam_j, valid_j, n):
    """n valid pixels of frame i, lifted, mapped by rel = (s, R, t) into the other sequence's frame and projected into frame j with
    the reference's rounding; those that land outside or on an invalid pixel are dropped, 20 % are replaced by random pixels, and
    each match is seen in a random generated view"""
    s, R, t = rel
    px = rng.choice(np.flatnonzero(valid_i), n, replace=False)
    q = s * (pts_i[px] @ R.T) + t
    pc = q @ np.asarray(cam_j.R).T + np.asarray(cam_j.t)
    u2 = np.trunc(cam_j.fx * pc[:, 0] / pc[:, 2] + cam_j.cx + 0.5).astype(np.int64)
    v2 = np.trunc(cam_j.fy * pc[:, 1] / pc[:, 2] + cam_j.cy + 0.5).astype(np.int64)
    ok = (u2 >= 0) & (u2 < SW) & (v2 >= 0) & (v2 < SH)
    ok[ok] = valid_j[v2[ok] * SW + u2[ok]].astype(bool)
    u1, v1, u2, v2 = px[ok] % SW, px[ok] // SW, u2[ok], v2[ok]
    m = len(u1)
    bad = rng.random(m) < 0.2
    u2, v2 = np.where(bad, rng.integers(0, SW, m), u2), np.where(bad, rng.integers(0, SH, m), v2)
    # base pixel -> the generated-view pixel whose tex entry it is: view 1 is shifted right by one, view 2 up by one (np.roll wraps)
    a1, a2 = rng.integers(0, VIEWS, m), rng.integers(0, VIEWS, m)
    g = lambda a, u, v: (np.where(a == 1, (u + 1) % SW, u), np.where(a == 2, (v - 1) % SH, v))
    (gu1, gv1), (gu2, gv2) = g(a1, u1, v1), g(a2, u2, v2)
    return np.stack([a1, gu1, gv1, a2, gu2, gv2], 1).astype(np.int32)


@functools.lru_cache(maxsize=1)
def world_frames():
    return S.make_sequence(6, SW, SH, 3.0)


def make_sequences(groups, samples=400, short=()):
    """the frames of S.make_sequence(6, 160, 120, 3.0) split into sequences (`groups` lists each sequence's frames), sequence k
    re-expressed by similarity(k); raw matches between adjacent sequences; `short` = the (sequence, i, j) buckets that hold fewer
    than min_match_count matches.  -> list of dict(cameras, depths, tex, imgs, raw, pts, valid), and the similarities."""
    cams, depths = world_frames()
    rng = np.random.default_rng(17)
    seqs, sims = [], [similarity(k) for k in range(len(groups))]
    for k, frames in enumerate(groups):
        s, R, t = sims[k]
        cd = [in_frame(cams[f], depths[f], s, R, t) for f in frames]
        d = np.stack([x[1] for x in cd])
        assert ((d == 0) | ((d >= S.MIN_DSP) & (d <= S.MAX_DSP))).all() and (d > 0).mean() > 0.05
        un = [O.depth_unproject(x[1], x[0], S.MIN_DSP, S.MAX_DSP) for x in cd]
        seqs.append(dict(cameras=[x[0] for x in cd], depths=d, tex=np.stack([tex_tables()] * len(frames)),
                         imgs=np.stack([image(f, rng) for f in frames]), pts=[u[0] for u in un], valid=[u[1] for u in un]))
    for k in range(len(groups) - 1):
        a, b = seqs[k], seqs[k + 1]
        (sa, Ra, ta), (sb, Rb, tb) = sims[k], sims[k + 1]
        rel = (sb / sa, Rb @ Ra.T, tb - (sb / sa) * (Rb @ Ra.T @ ta))                     # frame of k -> frame of k + 1
        a["rel"] = rel
        a["raw"] = [[raw_matches(rng, a["pts"][i], a["valid"][i], rel, b["cameras"][j], b["valid"][j], samples)[:(3 + i + j) if (k, i, j) in short else None]
                     for j in range(len(b["cameras"]))] for i in range(len(a["cameras"]))]
    return seqs, sims


def expected_pair(a, b, state):
    """one turn of the loop from the oracle's one-pair functions: match_filter per pair, depth_unproject per frame and a gather,
    select_keyframe_pair, the closed-form srt_fit on the selected pair's kept matches"""
    n1, n2 = len(a["cameras"]), len(b["cameras"])
    p = SEQ_PRM
    filt = [[O.match_filter(a["raw"][i][j], a["tex"][i], a["valid"][i], b["tex"][j], b["valid"][j], a["imgs"][i], b["imgs"][j], p["ssd_win"],
                            p["ssd_err"], p["sample_interval"]) for j in range(n2)] for i in range(n1)]
    lifted = [[np.concatenate([a["pts"][i][m[:, 1] * SW + m[:, 0]], b["pts"][j][m[:, 3] * SW + m[:, 2]]], 1) for j, (m, _) in enumerate(row)]
              for i, row in enumerate(filt)]
    sel = O.select_keyframe_pair(a["cameras"], b["cameras"], lifted, p["min_match_count"], p["ransac_iters"], p["pixel_err"], p["adapt_ratio"], state)
    out = dict(stage_counts=np.array([[c for _, c in row] for row in filt]), sel=sel)
    if sel["rc"] == 0:
        i, j = sel["frm_idx1"], sel["frm_idx2"]
        kept = lifted[i][j][sel["keep"][i][j]]
        out.update(matches=kept, fit=O.srt_fit(kept, a["cameras"][i], b["cameras"][j]))
    return out


@functools.lru_cache(maxsize=1)
def pair_scenario():
    seqs, sims = make_sequences([(0, 1, 2), (3, 4, 5)], short=((0, 0, 2), (0, 2, 0)))
    return seqs, expected_pair(seqs[0], seqs[1], 9)


def test_the_sequence_pair_scenario_selects_a_pair_and_recovers_the_truth():
    """the oracle alone, on the CPU side of the test: a pair is selected, the truth recovered, two buckets are too small"""
    seqs, want = pair_scenario()
    s, R, _ = seqs[0]["rel"]
    assert want["sel"]["rc"] == 0
    fs, fR, _, _ = want["fit"]
    print("oracle fit: scale", fs, "truth", s, "max |R - truth|", np.abs(fR - R).max(), "kept", len(want["matches"]))
    assert abs(fs / s - 1) < 0.02 and np.abs(fR - R).max() < 0.02
    sizes = want["stage_counts"][:, :, 2]
    assert (sizes < SEQ_PRM["min_match_count"]).sum() == 2 and (sizes > 100).sum() == 7


@pytest.mark.gpu
def test_sequence_pair(processor):
    seqs, want = pair_scenario()
    a, b = seqs
    g = processor.SequencePairSRT(a["cameras"], b["cameras"], a["depths"], b["depths"], a["raw"], a["tex"], b["tex"], a["imgs"], b["imgs"],
                                  state=9, **SEQ_PRM)
    sel = want["sel"]
    assert np.array_equal(g["stage_counts"], want["stage_counts"])
    assert np.array_equal(g["n_keep"], sel["n_keep"])
    assert (g["frm_idx1"], g["frm_idx2"]) == (sel["frm_idx1"], sel["frm_idx2"]) and g["state"] == sel["state"]
    assert len(g["matches"]) == len(want["matches"])
    assert np.abs(g["matches"] - want["matches"]).max() <= 1e-12
    os_, oR, ot, ores = want["fit"]
    print("scale", g["scale"] - os_, "R", np.abs(g["R"] - oR).max(), "t", np.abs(g["t"] - ot).max(), "residual", g["residual"], ores)
    assert abs(g["scale"] - os_) <= 1e-12 and np.abs(g["R"] - oR).max() <= 1e-11 and np.abs(g["t"] - ot).max() <= 1e-11
    assert abs(g["residual"] - ores) <= 1e-9 * max(1.0, abs(ores))
    s, R, _ = a["rel"]
    assert abs(g["scale"] / s - 1) < 0.02 and np.abs(g["R"] - R).max() < 0.02
    with pytest.raises(_lib.MvsError) as e:
        processor.SequencePairSRT(a["cameras"], b["cameras"], a["depths"], b["depths"], a["raw"], a["tex"], b["tex"], a["imgs"], b["imgs"],
                                  state=9, **dict(SEQ_PRM, min_match_count=10_000))
    assert e.value.code == -9


# -------------------------------------------------------------------- 3. chain ----
@functools.lru_cache(maxsize=1)
def chain_scenario():
    seqs, _ = make_sequences([(0, 1), (2, 3), (4, 5)])
    state, fits, select = 5, [], []
    for k in range(2):
        e = expected_pair(seqs[k], seqs[k + 1], state)
        assert e["sel"]["rc"] == 0
        state = e["sel"]["state"]
        fits.append(e["fit"])
        select.append((e["sel"]["frm_idx1"], e["sel"]["frm_idx2"]))
    scales, Rs, ts = [], [], []
    for k, (s, R, t, _) in enumerate(fits):                          # Processor.cpp:819-823
        for k0 in range(k):
            scales[k0], Rs[k0], ts[k0] = O.srt_compose(s, R, t, scales[k0], Rs[k0], ts[k0])
        scales.append(s); Rs.append(R); ts.append(t)
    scales.append(1.0); Rs.append(np.eye(3)); ts.append(np.zeros(3))  # :851-853
    return seqs, np.array(scales), np.array(Rs), np.array(ts), select, state


@pytest.mark.gpu
def test_chain(processor, tmp_path):
    seqs, scales, Rs, ts, select, state = chain_scenario()
    prm = {k: v for k, v in SEQ_PRM.items()}
    st = np.array([5], np.uint32)
    gs, gR, gt, gsel = processor.CalcSimilarityTransformationSeq(seqs, prm, st, srt_txt=tmp_path / "SRT.txt")
    assert gsel == select and int(st[0]) == state
    assert gs.shape == (3,) and gs[2] == 1.0 and np.array_equal(gR[2], np.eye(3)) and not gt[2].any()
    assert np.abs(gs - scales).max() <= 1e-12 and np.abs(gR - Rs).max() <= 1e-11 and np.abs(gt - ts).max() <= 1e-11
    mio.write_srt_txt(tmp_path / "want.txt", scales, Rs, ts)
    assert (tmp_path / "SRT.txt").read_bytes() == (tmp_path / "want.txt").read_bytes()
    # the chain is the input of the stitch tail: a few points of every sequence through StitchPointSets
    paths = []
    for k, q in enumerate(seqs):
        p = np.concatenate([pts[np.flatnonzero(v)[::97]] for pts, v in zip(q["pts"], q["valid"])])
        paths.append(tmp_path / f"seq{k}.npts")
        mio.write_npts(paths[-1], p, np.tile([0.0, 0.0, 1.0], (len(p), 1)))
    cams = [q["cameras"] for q in seqs]
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    got = processor.StitchPointSets(paths, gs, gR, gt, cams, tmp_path / "a")
    want = processor.StitchPointSets(paths, scales, Rs, ts, cams, tmp_path / "b")
    assert len(got) == 3 and np.array_equal(got, want)
