"""Host side of mvs_srt_refine (include/mvs.h): symbols, the layout and defaults of mvs_srt_refine_params, the argument checks of both
entries (they run before a device is needed), the file entry's errors, what the scenes of tests/srt_refine_scenes.py must hold, the
restatement tests/ref_srt_refine.py on scene H against the truth and on scenes T and E against unquantised sums, and the shared rules
header (csrc/srt_refine_rules.h) as a stand-alone program under the address and undefined-behaviour sanitizers against the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P
from tests import ref_srt_refine as R, srt_refine_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE, E_IO = -1, -4, -10


def _call(fn="mvs_srt_refine", n_seq=2, off=None, null=(), scales=None, Rs=None, ts=None, prm=True, **fields):
    off = np.asarray([0, 4, 8, 12, 16][:n_seq + 1] if off is None else off, np.int64)
    m = max(n_seq, 4)
    pts, nrm = np.zeros((16, 3)), np.zeros((16, 3))
    s = np.ones(m) if scales is None else np.asarray(scales, np.float64)
    Rm = np.tile(np.eye(3), (m, 1, 1)) if Rs is None else np.asarray(Rs, np.float64)
    t = np.zeros((m, 3)) if ts is None else np.asarray(ts, np.float64)
    done, hist, pc = C.c_int32(-7), np.zeros((64, 2)), np.zeros((m, m), np.int64)
    p = P.srt_refine_params(**fields)
    args = dict(points=L.ptr(pts), normals=L.ptr(nrm), seg_off=L.ptr(off), n_seq=n_seq, scales=L.ptr(s), R=L.ptr(Rm), t=L.ptr(t),
                p=C.byref(p) if prm else None, iters_done=C.byref(done), history=L.ptr(hist), pair_count=L.ptr(pc))
    for k in null:
        args[k] = None
    return getattr(L.lib(), fn)(*args.values(), *((None,) if fn.endswith("_dev") else ()))


def test_symbols_and_params_layout():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_srt_refine_default_params", "mvs_srt_refine", "mvs_srt_refine_dev", "mvs_processor_refine_srt", "mvs_test_srt_refine_sums",
                 "mvs_test_srt_refine_timed"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T = L.CSrtRefineParams
    assert C.sizeof(T) == 56
    assert [k for k, _ in T._fields_] == ["rel_dist", "min_cos", "damping", "tol", "iters", "stride", "fixed_seq", "min_pairs", "flags", "reserved"]
    assert [getattr(T, k).offset for k, _ in T._fields_] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    p = P.srt_refine_params()
    got = (p.rel_dist, p.min_cos, p.damping, p.tol, p.iters, p.stride, p.fixed_seq, p.min_pairs, p.flags, p.reserved)
    assert got == (0.02, 0.7, 1e-9, 1e-9, 20, 1, -1, 64, 0, 0)
    ref = R.params()
    assert tuple(ref[k] for k, _ in T._fields_[:9]) == got[:9]
    assert L.SRT_REFINE_FIX_SCALE == R.FIX_SCALE == 1 and L.SRT_REFINE_TERMS == R.TERMS == 121
    q = P.srt_refine_params(rel_dist=0.05, stride=3, flags=1)
    assert (q.rel_dist, q.stride, q.flags) == (0.05, 3, 1)
    assert lib.mvs_abi_version() == 4
    with pytest.raises(L.MvsError):
        P.srt_refine_params(levels=3)


_nan_R = np.tile(np.eye(3), (4, 1, 1))
_nan_R[1, 2, 0] = math.nan
BAD = [dict(null=("points",)), dict(null=("normals",)), dict(null=("seg_off",)), dict(null=("scales",)), dict(null=("R",)), dict(null=("t",)),
       dict(null=("iters_done",)), dict(n_seq=1), dict(n_seq=0), dict(n_seq=-3), dict(off=[1, 4, 8]), dict(off=[0, 8, 4]),
       dict(off=[0, 4, 2 ** 31 - 1]), dict(off=[0, 4, 2 ** 24 + 5]), dict(off=[0, 4, 3 * 2 ** 24 + 5], stride=3),
       dict(rel_dist=0.0), dict(rel_dist=-0.02), dict(rel_dist=1.5), dict(rel_dist=math.nan), dict(rel_dist=math.inf),
       dict(min_cos=-1.5), dict(min_cos=1.0000001), dict(min_cos=math.nan), dict(damping=-1e-9), dict(damping=math.nan), dict(damping=math.inf),
       dict(tol=-1.0), dict(tol=math.nan), dict(tol=math.inf), dict(iters=0), dict(iters=65), dict(iters=-1), dict(stride=0), dict(stride=-2),
       dict(fixed_seq=2), dict(fixed_seq=-2), dict(min_pairs=-1), dict(flags=2), dict(flags=3), dict(flags=-1), dict(reserved=1), dict(reserved=-1),
       dict(scales=[1.0, 0.0, 1.0, 1.0]), dict(scales=[-1.0, 1.0, 1.0, 1.0]), dict(scales=[1.0, math.inf, 1.0, 1.0]), dict(scales=[math.nan, 1.0, 1.0, 1.0]),
       dict(Rs=_nan_R), dict(ts=[[0, 0, 0], [0, math.inf, 0], [0, 0, 0], [0, 0, 0]])]


def _id(kw):
    return ",".join(f"{k}={'nan-R' if k == 'Rs' else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BAD, ids=[_id(kw) for kw in BAD])
def test_argument_errors_need_no_device(kw):
    assert _call(**kw) == E_INVALID
    assert b"mvs_srt_refine:" in L.lib().mvs_last_error()
    assert _call(fn="mvs_srt_refine_dev", **kw) == E_INVALID
    assert b"mvs_srt_refine_dev:" in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    # the arrays of _call live on the host: with a device present the _dev form would hand them to a kernel, so it is called only where
    # the answer is MVS_E_NO_DEVICE (tests/test_gpu_srt_refine.py holds the device form on device arrays).  All points are at the origin:
    # with a device the call gets as far as I2 and reports that there is no box.
    ok = (E_NO_DEVICE,) if L.device_count() == 0 else (-9,)
    for fn in ("mvs_srt_refine",) + (("mvs_srt_refine_dev",) if L.device_count() == 0 else ()):
        assert _call(fn=fn) in ok
        assert _call(fn=fn, prm=False) in ok                                                   # NULL params: the defaults
        assert _call(fn=fn, null=("history", "pair_count")) in ok
        assert _call(fn=fn, n_seq=4, fixed_seq=3, iters=64, stride=7, flags=1, min_cos=-1.0, rel_dist=1.0, damping=0.0, tol=0.0, min_pairs=0) in ok
        assert _call(fn=fn, off=[0, 0, 16]) in ok                                              # an empty sequence
    if L.device_count() == 0:                                                                  # 2^24 queries pass the checks (the arrays are never read)
        assert _call(off=[0, 4, 3 * 2 ** 24 - 5], stride=3) == E_NO_DEVICE


def test_python_entries_check_their_shapes():
    pts = [np.zeros((4, 3)), np.zeros((5, 3))]
    s, Rm, t = np.ones(2), np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
    for bad in (dict(points=pts[:1]), dict(normals=[np.zeros((4, 3)), np.zeros((4, 3))]), dict(points=[np.zeros((4, 2)), np.zeros((5, 3))]),
                dict(Rs=np.zeros((3, 3, 3)))):
        kw = dict(points=pts, normals=pts, scales=s, Rs=Rm, ts=t)
        kw.update(bad)
        with pytest.raises((L.MvsError, ValueError)):
            P.RefineSRT(**kw)


def test_the_file_entry_reports_its_errors(tmp_path):
    """the files are read before a device is needed: a missing or short one is MVS_E_IO naming it; nothing is written then"""
    sc = SC.scene("T")
    paths = [str(tmp_path / f"s{k}.npts") for k in range(2)]
    for k in range(2):
        IO.write_npts(paths[k], sc["points"][k], sc["normals"][k])
    srt, out = str(tmp_path / "SRT.txt"), str(tmp_path / "SRT_refined.txt")
    IO.write_srt_txt(srt, sc["scales"], sc["Rs"], sc["ts"])
    with pytest.raises(L.MvsError) as e:
        P.RefineSRTFiles([paths[0], str(tmp_path / "none.npts")], srt, out)
    assert e.value.code == E_IO and "none.npts" in str(e.value)
    with pytest.raises(L.MvsError) as e:
        P.RefineSRTFiles(paths, str(tmp_path / "none.txt"), out)
    assert e.value.code == E_IO and "none.txt" in str(e.value)
    IO.write_srt_txt(str(tmp_path / "short.txt"), sc["scales"][:1], sc["Rs"][:1], sc["ts"][:1])
    with pytest.raises(L.MvsError) as e:
        P.RefineSRTFiles(paths, str(tmp_path / "short.txt"), out)
    assert e.value.code == E_IO and "short.txt" in str(e.value)
    with pytest.raises(L.MvsError) as e:
        P.RefineSRTFiles(paths, srt, out, P.srt_refine_params(rel_dist=0.0))
    assert e.value.code == E_INVALID and "mvs_processor_refine_srt:" in str(e.value)
    with pytest.raises(L.MvsError) as e:
        P.RefineSRTFiles(paths[:1], srt, out)
    assert e.value.code == E_INVALID
    lib = L.lib()
    arr = (C.c_char_p * 2)(*[os.fsencode(p) for p in paths])
    done = C.c_int32(0)
    args = lambda **kw: tuple({**dict(n=2, paths=arr, i=os.fsencode(srt), p=None, o=os.fsencode(out), d=C.byref(done), h=None), **kw}.values())
    for kw in (dict(paths=None), dict(i=None), dict(o=None), dict(d=None), dict(n=1), dict(paths=(C.c_char_p * 2)(os.fsencode(paths[0]), None))):
        assert lib.mvs_processor_refine_srt(*args(**kw)) == E_INVALID
        assert b"mvs_processor_refine_srt:" in lib.mvs_last_error()
    if L.device_count() == 0:
        assert lib.mvs_processor_refine_srt(*args()) == E_NO_DEVICE
    assert not os.path.exists(out)


# ------------------------------------------------------------------ the scenes and the restatement ----
def test_scenes_hold_what_they_are_there_for():
    sc = SC.scene("H")
    assert [len(p) for p in sc["points"]] == [576, 576, 576] and list(sc["true"][0]) == [1.3, 0.8, 1.0]
    for k in range(2):                                                                          # about 2 degrees, 0.02 and 2 %
        dR = sc["Rs"][k] @ sc["true"][1][k].T
        assert abs(math.degrees(math.acos((np.trace(dR) - 1) / 2)) - 2.0) < 1e-6
        assert abs(abs(sc["scales"][k] / sc["true"][0][k] - 1) - 0.02) < 1e-12
    # T: every step is exact, the ties and thresholds are there
    sc = SC.scene("T")
    S, c, D, det = SC.first_search("T")
    assert list(c) == [0.0, 0.0, 0.0] and D == 12.0
    for k in range(2):
        assert np.array_equal(sc["points"][k].astype(np.float32).astype(np.float64), sc["points"][k])
        assert np.array_equal(R.seq_apply(sc["scales"][k], sc["Rs"][k], sc["ts"][k], sc["points"][k]), sc["world"][k])
    f = det[(0, 1)]
    assert list(f["query"]) == [0, 1, 2, 3, 5, 7, 8] and list(f["target"]) == [0, 2, 6, 8, 10, 12, 12]
    assert list(f["tie"]) == [True, True, True, False, False, False, False]                     # two, four, coincident: the lower index
    assert f["at_cap"] == 1 and f["searched"] == 9                                              # 3 sits at the cap; 4 (beyond) and 6 (opposite) are rejected
    assert f["cos"][4] == 0.0 and f["r"][2] == 0.0                                              # min_cos met by a dot product of 0; the coincident match
    b = det[(1, 0)]
    assert b["tie"][list(b["query"]).index(12)] and b["target"][list(b["query"]).index(12)] == 7
    assert 13 not in b["query"] and 14 not in b["query"]                                        # the corners of the box match nothing
    # E
    sc = SC.scene("E")
    assert [len(p) for p in sc["points"]] == [130, 65, 1] and sc["params"]["stride"] == 3
    S, c, D, det = SC.first_search("E")
    assert (~R.usable(sc["points"][0])).sum() == 4 and (~R.usable(sc["points"][1])).sum() == 4
    assert det[(1, 0)]["searched"] == 22 - 3 and det[(0, 1)]["searched"] == 44 - 1              # bad queries search nothing
    assert 6 not in det[(1, 0)]["query"] and len(det[(1, 0)]["query"]) >= 8                     # the zero normal rejects its match
    assert all(len(det[k]["query"]) == 0 for k in ((0, 2), (2, 0), (1, 2), (2, 1)))             # sequence 2 overlaps nothing
    ref = SC.reference("E")
    assert ref["iters_done"] >= 1
    assert np.array_equal(ref["Rs"][2], sc["Rs"][2]) and np.array_equal(ref["ts"][2], sc["ts"][2]) and ref["scales"][2] == sc["scales"][2]
    assert np.array_equal(ref["Rs"][0], sc["Rs"][0]) and not np.array_equal(ref["Rs"][1], sc["Rs"][1])


def test_restatement_on_scene_h_pulls_the_chain_to_the_truth():
    """the final rms distance of the mapped points to the truth is at most 1/4 of the starting one"""
    sc, ref = SC.scene("H"), SC.reference("H")
    start, end = SC.rms_to_truth(sc, sc["scales"], sc["Rs"], sc["ts"]), SC.rms_to_truth(sc, ref["scales"], ref["Rs"], ref["ts"])
    print(f"rms to truth {start:.6f} -> {end:.6f} in {ref['iters_done']} iterations; history {ref['history'].tolist()}")
    assert end <= start / 4
    assert 1 <= ref["iters_done"] < 20 and len(ref["history"]) == ref["iters_done"]              # tol ended the call
    assert ref["history"][-1, 1] < ref["history"][0, 1] / 4
    assert ref["scales"][2] == 1.0 and np.array_equal(ref["Rs"][2], np.eye(3)) and not ref["ts"][2].any()   # the last sequence is fixed


def test_fix_scale_returns_the_scales_bit_unchanged():
    sc = SC.scene("H")
    ref = R.refine(sc["points"], sc["normals"], sc["scales"], sc["Rs"], sc["ts"], R.params(rel_dist=0.05, flags=R.FIX_SCALE, iters=3))
    assert ref["iters_done"] == 3
    assert ref["scales"].tobytes() == np.asarray(sc["scales"], np.float64).tobytes()
    assert not np.array_equal(ref["Rs"][0], sc["Rs"][0])


@pytest.mark.parametrize("name", ("T", "E"))
def test_quantised_sums_stay_within_the_rounding_bound(name):
    """every sum of the restatement is within count * 2^-37 of the same sum in unquantised fp64: the rounding bound of q"""
    S, _, _, _ = SC.first_search(name)
    X, _, _, _ = SC.first_search(name, True)
    n, seen = len(S), 0
    for a in range(n):
        for b in range(n):
            cnt = S[a][b][0]
            assert cnt == X[a][b][0]
            for k in range(1, R.TERMS):
                assert abs(float(S[a][b][k]) / R.Q - X[a][b][k]) <= cnt * 2.0 ** -37
                seen += cnt > 0
    assert seen >= 2 * 120


# ------------------------------------------------------------------ the shared rules ----
def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "srt_refine_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "srt_refine_rules.cpp"), "-o", exe])
    return exe


def write_scene(path, sc):
    """the input of tests/srt_refine_rules.cpp"""
    n, p = len(sc["points"]), sc["params"]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(q) for q in sc["points"]])
    with open(path, "wb") as fh:
        fh.write(np.asarray([n, p["stride"]], np.int32).tobytes())
        fh.write(np.asarray([p["rel_dist"], p["min_cos"]], np.float64).tobytes())
        fh.write(off.tobytes())
        for k in range(n):
            fh.write(np.concatenate([[sc["scales"][k]], np.asarray(sc["Rs"][k], np.float64).reshape(9), np.asarray(sc["ts"][k], np.float64).reshape(3)]).tobytes())
        fh.write(np.ascontiguousarray(np.concatenate(sc["points"]), np.float64).tobytes())
        fh.write(np.ascontiguousarray(np.concatenate(sc["normals"]), np.float64).tobytes())


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """tests/srt_refine_rules.cpp: the header's own cases, then I1-I6 on scenes T and E with a brute-force search, on heap blocks of exact
    size: the sums equal the restatement's integers exactly (host code, no contraction)"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "srt refine rules ok" in run.stdout, run.stdout + run.stderr
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for name in ("T", "E"):
        sc = SC.scene(name)
        S, _, _, _ = SC.first_search(name)
        write_scene(fin, sc)
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        n = len(sc["points"])
        got = np.fromfile(fout, np.int64).reshape(n, n, R.TERMS)
        assert np.array_equal(got, SC.flat(S)), name
