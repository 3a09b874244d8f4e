"""mvs_srt_refine on the GPU against the restatement (tests/ref_srt_refine.py) on the scenes of tests/srt_refine_scenes.py: the 121 int64
sums of every pair exactly; the step iteration by iteration; the whole call against the truth; pair counts, the held sequence, equal
bytes of two runs, the device form on a stream and the file form."""
import ctypes as C
import functools

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P
from tests import ref_srt_refine as R, srt_refine_scenes as SC

pytestmark = pytest.mark.gpu


def _prm(p, **kw):
    return P.srt_refine_params(**{**{k: v for k, v in p.items()}, **kw})


def _hook(sc, scales, Rs, ts, p):
    """mvs_test_srt_refine_sums -> (sums int64 [n, n, 121], c_D [4])"""
    n = len(sc["points"])
    pts, nrm = np.ascontiguousarray(np.concatenate(sc["points"])), np.ascontiguousarray(np.concatenate(sc["normals"]))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(q) for q in sc["points"]])
    s, Rm, t = L.arr(scales, np.float64).reshape(n), L.arr(Rs, np.float64).reshape(n, 3, 3), L.arr(ts, np.float64).reshape(n, 3)
    sums, cD = np.full((n, n, R.TERMS), -1, np.int64), np.zeros(4)
    prm = _prm(p)
    L.check(L.lib().mvs_test_srt_refine_sums(L.ptr(pts), L.ptr(nrm), L.ptr(off), n, L.ptr(s), L.ptr(Rm), L.ptr(t), C.byref(prm), L.ptr(sums), L.ptr(cD)))
    return sums, cD


@functools.lru_cache(maxsize=None)
def _gpu(name):
    """the whole call on the scene with the scene's parameters, once per process (do not modify the result)"""
    sc = SC.scene(name)
    return P.RefineSRT(sc["points"], sc["normals"], sc["scales"], sc["Rs"], sc["ts"], _prm(sc["params"]))


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() <= rel * np.abs(want).max()


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_sums_of_every_pair_equal_the_restatement(name):
    sc = SC.scene(name)
    S, c, D, _ = SC.first_search(name)
    sums, cD = _hook(sc, sc["scales"], sc["Rs"], sc["ts"], sc["params"])
    assert np.array_equal(cD[:3], c) and cD[3] == D
    want = SC.flat(S)
    print(name, "accepted matches per pair", sums[:, :, 0].tolist())
    assert np.array_equal(sums[:, :, 0], want[:, :, 0])
    assert np.array_equal(sums, want)
    assert want[:, :, 0].sum() > 0


def test_scene_h_iteration_by_iteration():
    """iters = 1 from the restatement's chain at each of its first six iterations: the sums are the restatement's integers every time,
    so only libm's exp, sin, cos and a dozen fp64 operations can differ in the step: the chain is within 1e-12 relative of the
    restatement's update (a wrong rule shows at 1e-6 or more)"""
    sc, ref = SC.scene("H"), SC.reference("H")
    assert len(ref["trace"]) >= 6
    for it, (before, _, _) in enumerate(ref["trace"][:6]):
        # a call of its own from that chain: I2 takes the frame from the chain the call is given
        one = R.refine(sc["points"], sc["normals"], *before, R.params(**{**sc["params"], "iters": 1}))
        (_, S, after), = one["trace"]
        assert after is not None and one["iters_done"] == 1
        sums, cD = _hook(sc, *before, sc["params"])
        assert np.array_equal(cD[:3], one["c"]) and cD[3] == one["D"]
        assert np.array_equal(sums, SC.flat(S)), it
        s, Rm, t, rep = P.RefineSRT(sc["points"], sc["normals"], *before, _prm(sc["params"], iters=1))
        assert rep["iters_done"] == 1
        worst = max(np.abs(np.asarray(g) - np.asarray(w)).max() / np.abs(np.asarray(w)).max() for g, w in zip((s, Rm, t), after))
        print(f"iteration {it}: largest relative difference of the updated chain {worst:.3e}")
        assert _close(s, after[0]) and _close(Rm, after[1]) and _close(t, after[2]), it
        assert rep["history"][0, 0] == one["history"][0, 0] and _close(rep["history"][0, 1], one["history"][0, 1], 1e-12)
        assert np.array_equal(rep["pair_count"], SC.flat(S)[:, :, 0])


def test_the_full_call_on_scene_h_meets_the_truth():
    sc, ref = SC.scene("H"), SC.reference("H")
    s, Rm, t, rep = _gpu("H")
    start, end = SC.rms_to_truth(sc, sc["scales"], sc["Rs"], sc["ts"]), SC.rms_to_truth(sc, s, Rm, t)
    print(f"rms to truth {start:.6f} -> {end:.6f} in {rep['iters_done']} iterations (restatement: {ref['iters_done']})")
    assert end <= start / 4
    assert 1 <= rep["iters_done"] <= 20 and rep["history"].shape == (rep["iters_done"], 2)
    assert s[2] == 1.0 and np.array_equal(Rm[2], np.eye(3)) and not t[2].any()                   # the last sequence does not move
    assert not np.shares_memory(s, sc["scales"]) and s[0] != sc["scales"][0]


def test_pair_counts_on_scenes_t_and_e():
    for name in ("T", "E"):
        ref = SC.reference(name)
        _, _, _, rep = _gpu(name)
        if name == "T":                                                                          # too few matches: every sequence is held
            assert rep["iters_done"] == 0 == ref["iters_done"]
            assert np.array_equal(rep["pair_count"], ref["pair_count"])
        else:
            # the last search of a 20-iteration call sees a chain that differs from the restatement's in its last bits; the first
            # search sees the same chain
            sc = SC.scene(name)
            _, _, _, one = P.RefineSRT(sc["points"], sc["normals"], sc["scales"], sc["Rs"], sc["ts"], _prm(sc["params"], iters=1))
            assert np.array_equal(one["pair_count"], SC.flat(SC.first_search(name)[0])[:, :, 0])
            print("E: pair counts of the last search", rep["pair_count"].tolist(), "restatement", ref["pair_count"].tolist())
            assert rep["iters_done"] == ref["iters_done"] and np.array_equal(rep["pair_count"], ref["pair_count"])
            assert rep["pair_count"][2].sum() == 0 and rep["pair_count"][:, 2].sum() == 0


def test_scene_t_returns_the_chain_unchanged():
    sc = SC.scene("T")
    s, Rm, t, rep = _gpu("T")
    assert rep["iters_done"] == 0 and rep["history"].shape == (0, 2)
    assert s.tobytes() == sc["scales"].tobytes() and Rm.tobytes() == sc["Rs"].tobytes() and t.tobytes() == sc["ts"].tobytes()


def test_the_held_sequence_of_scene_e_keeps_its_bytes():
    sc = SC.scene("E")
    s, Rm, t, rep = _gpu("E")
    assert rep["iters_done"] >= 1
    for k in (0, 2):                                                                             # 0 is fixed, 2 matches nothing and is held
        assert s[k:k + 1].tobytes() == sc["scales"][k:k + 1].tobytes()
        assert Rm[k].tobytes() == sc["Rs"][k].tobytes() and t[k].tobytes() == sc["ts"][k].tobytes()
    assert not np.array_equal(Rm[1], sc["Rs"][1]) and s[1] != sc["scales"][1]
    with_fix = P.RefineSRT(sc["points"], sc["normals"], sc["scales"], sc["Rs"], sc["ts"], _prm(sc["params"], flags=L.SRT_REFINE_FIX_SCALE, iters=2))
    assert with_fix[0].tobytes() == sc["scales"].tobytes() and not np.array_equal(with_fix[1][1], sc["Rs"][1])


def test_two_runs_give_the_same_bytes():
    for name in ("H", "E"):
        sc = SC.scene(name)
        a = _gpu(name)
        b = P.RefineSRT(sc["points"], sc["normals"], sc["scales"], sc["Rs"], sc["ts"], _prm(sc["params"]))
        for x, y in zip(a[:3], b[:3]):
            assert x.tobytes() == y.tobytes()
        assert a[3]["iters_done"] == b[3]["iters_done"] and a[3]["history"].tobytes() == b[3]["history"].tobytes()
        assert np.array_equal(a[3]["pair_count"], b[3]["pair_count"])


def test_the_device_form_on_a_stream_equals_the_host_form():
    import torch
    for name in ("H", "E"):
        sc = SC.scene(name)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            pts = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in sc["points"]]
            nrm = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in sc["normals"]]
        assert torch.cuda.current_stream() != st                    # the inputs are pending on st; the call must order itself there
        dev = P.RefineSRT(pts, nrm, sc["scales"], sc["Rs"], sc["ts"], _prm(sc["params"]), stream=st.cuda_stream)
        host = _gpu(name)
        for x, y in zip(dev[:3], host[:3]):
            assert isinstance(x, np.ndarray) and x.tobytes() == y.tobytes()
        assert dev[3]["iters_done"] == host[3]["iters_done"] and dev[3]["history"].tobytes() == host[3]["history"].tobytes()
        assert np.array_equal(dev[3]["pair_count"], host[3]["pair_count"])


def test_the_file_form_equals_the_array_form_on_what_the_files_hold(tmp_path):
    sc = SC.scene("H")
    paths = [str(tmp_path / f"s{k}.npts") for k in range(3)]
    for k in range(3):
        IO.write_npts(paths[k], sc["points"][k], sc["normals"][k])
    srt, out, want_txt = str(tmp_path / "SRT.txt"), str(tmp_path / "SRT_refined.txt"), str(tmp_path / "want.txt")
    IO.write_srt_txt(srt, sc["scales"], sc["Rs"], sc["ts"])
    prm = _prm(sc["params"], iters=4)
    rep = P.RefineSRTFiles(paths, srt, out, prm)
    held = [IO.read_npts(p) for p in paths]
    s0, R0, t0 = IO.read_srt_txt(srt, 3)
    s, Rm, t, want = P.RefineSRT([h[0] for h in held], [h[1] for h in held], s0, R0, t0, prm)
    assert rep["iters_done"] == want["iters_done"] == 4 and rep["history"].tobytes() == want["history"].tobytes()
    IO.write_srt_txt(want_txt, s, Rm, t)
    assert open(out, "rb").read() == open(want_txt, "rb").read()
    got = IO.read_srt_txt(out, 3)
    assert SC.rms_to_truth(sc, *got) <= SC.rms_to_truth(sc, s0, R0, t0) / 4                      # float32 points and a %g chain still get there
