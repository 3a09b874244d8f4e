"""Host side of mvs_recover_depth_maps_aggregated (include/mvs.h, rules S1-S6): symbols, the layout and the defaults of
mvs_depth_aggregate_params, every argument check of the four C entries (they run before a device is needed), properties of the numpy
restatement tests/ref_depth_sgm.py, the conditions the scenes of tests/depth_sgm_scenes.py must meet for the GPU comparison to be exact,
the recorded quality numbers, and the shared rules header (csrc/depth_sgm_rules.h) as a stand-alone program under the address and
undefined-behaviour sanitizers — on its own cases and on the scenes A33 and STRIP, byte for byte against the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import depth_sgm_scenes as G, ref_depth_recover as R, ref_depth_sgm as A
from tests.test_depth_recover_host import BAD as BAD_PLAIN, _cam, _id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE, E_IO = -1, -4, -10
A_FIELDS = ("p1", "p2", "cost_cap", "paths", "max_volume_mb", "reserved")
A_NAMES = dict({k: k for k in A_FIELDS[:5]}, areserved="reserved")          # how _call names the fields of the aggregation
ENTRIES = ("mvs_recover_depth_maps_aggregated", "mvs_recover_depth_maps_aggregated_dev")
FILE_ENTRIES = ("mvs_processor_recover_depths_aggregated", "mvs_processor_recover_depths_aggregated_files")


def _call(cams=None, off=None, n_seq=1, cam_off=True, cam_ptr=True, imgs=True, prm=True, out=True, aprm=True, fn=ENTRIES[0], **fields):
    cams = [_cam(), _cam()] if cams is None else cams
    off = np.asarray([0, len(cams)] if off is None else off, np.int32)
    arr = (L.CCamera * max(1, len(cams)))(*[L.CCamera.of(c) for c in cams])
    px = max(1, sum(min(c.w, 64) * min(c.h, 64) for c in cams if c.w > 0 and c.h > 0))
    o, im = np.zeros(px, np.float32), np.zeros(3 * px, np.uint8)
    p = P.depth_recover_params(**{k: v for k, v in fields.items() if k not in A_NAMES})            # `reserved` is the plain sweep's
    a = P.depth_aggregate_params(**{A_NAMES[k]: v for k, v in fields.items() if k in A_NAMES})
    args = (n_seq, L.ptr(off) if cam_off else None, arr if cam_ptr else None, L.ptr(im) if imgs else None, C.byref(p) if prm else None,
            C.byref(a) if aprm else None, L.ptr(o) if out else None, None, None, None, None)
    return getattr(L.lib(), fn)(*args, *((None,) if fn.endswith("_dev") else ()))


def _call_file(fn, seq_dir, cams=None, off=None, n_seq=1, cam_off=True, cam_ptr=True, imgs=True, prm=True, aprm=True, dirs=True, **fields):
    """the same arguments through a file entry: ``seq_dir`` exists and holds no frame, so that nothing but an argument check can answer
    MVS_E_INVALID_ARG — a call that gets past the checks of the _files form ends in MVS_E_IO at 00000.jpg"""
    cams = [_cam(), _cam()] if cams is None else cams
    off = np.asarray([0, len(cams)] if off is None else off, np.int32)
    arr = (L.CCamera * max(1, len(cams)))(*[L.CCamera.of(c) for c in cams])
    px = max(1, sum(min(c.w, 64) * min(c.h, 64) for c in cams if c.w > 0 and c.h > 0))
    im = np.zeros(3 * px, np.uint8)
    p = P.depth_recover_params(**{k: v for k, v in fields.items() if k not in A_NAMES})
    a = P.depth_aggregate_params(**{A_NAMES[k]: v for k, v in fields.items() if k in A_NAMES})
    dd = (C.c_char_p * max(1, n_seq))(*[os.fsencode(str(seq_dir))] * max(1, n_seq))
    args = (n_seq, dd if dirs else None, L.ptr(off) if cam_off else None, arr if cam_ptr else None) + \
        ((L.ptr(im) if imgs else None,) if fn == FILE_ENTRIES[0] else ()) + (C.byref(p) if prm else None, C.byref(a) if aprm else None)
    return getattr(L.lib(), fn)(*args)


def test_symbols_layout_and_defaults():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_depth_aggregate_default_params",) + ENTRIES + ("mvs_processor_recover_depths_aggregated",
                                                                     "mvs_processor_recover_depths_aggregated_files"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T = L.CDepthAggregateParams
    assert C.sizeof(T) == 24
    assert [k for k, _ in T._fields_] == list(A_FIELDS) and [getattr(T, k).offset for k in A_FIELDS] == [0, 4, 8, 12, 16, 20]
    a = P.depth_aggregate_params()
    assert {k: getattr(a, k) for k in A_FIELDS} == A.aparams() == dict(p1=8, p2=128, cost_cap=255, paths=8, max_volume_mb=0, reserved=0)
    assert P.depth_aggregate_params(paths=4, p1=0).paths == 4
    with pytest.raises(L.MvsError):
        P.depth_aggregate_params(levels=3)
    assert lib.mvs_abi_version() == 4
    lib.mvs_depth_aggregate_default_params(None)                     # a NULL pointer is ignored, as by the other default calls


# every check of the plain sweep but its NULL params (tested below: the new entries have two), and the new ones.  A 16 x 12 frame with
# N = 7 has a rectangle of 2 x -2: nothing to hold; the budget cases use N = 0
BAD = [kw for kw in BAD_PLAIN if kw != dict(prm=False)] + [
    dict(prm=False), dict(p1=-1), dict(p1=129), dict(p1=9, p2=8), dict(p2=4096), dict(p1=4096, p2=4096), dict(p2=-1), dict(cost_cap=0), dict(cost_cap=-1),
    dict(cost_cap=4096), dict(paths=0), dict(paths=2), dict(paths=6), dict(paths=16), dict(paths=-8), dict(max_volume_mb=-1), dict(areserved=1),
    dict(areserved=-1),
    dict(cams=[_cam(w=1024, h=1024)], ssd_win=0, levels=1024, max_volume_mb=4095)]           # 4 * 2^20 * 1024 bytes = 4096 MB for one frame


@pytest.mark.parametrize("kw", BAD, ids=[_id(kw) for kw in BAD])
def test_argument_errors_need_no_device(kw):
    for fn in ENTRIES:
        assert _call(fn=fn, **kw) == E_INVALID
        assert (fn + ":").encode() in L.lib().mvs_last_error()


# what a file entry cannot be asked: it has no out, NULL params are the defaults, and the _files form has no imgs
BAD_FILE = [kw for kw in BAD if kw not in (dict(out=False), dict(prm=False))] + [dict(dirs=False), dict(p1=4095, p2=4096), dict(p2=5000)]


@pytest.mark.parametrize("kw", BAD_FILE, ids=[_id(kw) for kw in BAD_FILE])
def test_argument_errors_of_the_file_entries_come_before_any_frame_is_read(kw, tmp_path):
    for fn in FILE_ENTRIES:
        if fn == FILE_ENTRIES[1] and kw == dict(imgs=False):
            continue
        assert _call_file(fn, tmp_path, **kw) == E_INVALID, L.lib().mvs_last_error()
        assert (fn + ":").encode() in L.lib().mvs_last_error()
        assert not (tmp_path / "DATA").exists()


def test_the_file_entries_get_past_the_checks_with_valid_arguments(tmp_path):
    """the directory holds no frame: the _files form then reports the first one it misses, which shows that E_INVALID above is the answer
    of a check and not of the missing file"""
    for kw in (dict(), dict(prm=False), dict(aprm=False), dict(p1=0, p2=0, cost_cap=1, paths=4, max_volume_mb=1, ssd_win=0),
               dict(p1=4095, p2=4095, cost_cap=4095, max_volume_mb=2147483647)):
        assert _call_file(FILE_ENTRIES[1], tmp_path, **kw) == E_IO and b"00000.jpg" in L.lib().mvs_last_error()
        assert _call_file(FILE_ENTRIES[0], tmp_path, **kw) in (0, E_NO_DEVICE)


def test_the_budget_message_names_the_megabytes_of_one_frame(tmp_path):
    """1024 x 1024 pixels at N = 0 and 1024 levels are 4 * 2^30 bytes: 4096 MB, what the default budget holds"""
    big = dict(ssd_win=0, levels=1024)
    assert _call(cams=[_cam(w=1024, h=1024)], max_volume_mb=4095, **big) == E_INVALID
    assert b"need 4096 MB" in L.lib().mvs_last_error() and b"budget is 4095 MB" in L.lib().mvs_last_error()
    assert _call(cams=[_cam(w=1025, h=1024)], **big) == E_INVALID                        # the default budget
    assert b"need 4100 MB" in L.lib().mvs_last_error() and b"budget is %d MB" % L.SGM_VOLUME_MB in L.lib().mvs_last_error()
    for fn in FILE_ENTRIES:                                                              # the file forms say the same, under their names
        assert _call_file(fn, tmp_path, cams=[_cam(w=1024, h=1024)], max_volume_mb=4095, **big) == E_INVALID
        assert (fn + ":").encode() in L.lib().mvs_last_error() and b"need 4096 MB" in L.lib().mvs_last_error()
        assert _call_file(fn, tmp_path, cams=[_cam(w=1025, h=1024)], **big) == E_INVALID and b"need 4100 MB" in L.lib().mvs_last_error()
    assert _call(cams=[_cam(), _cam()], max_volume_mb=1, levels=1024, ssd_win=0, off=[0, 2]) in (0, E_NO_DEVICE)      # 16 x 12 x 1024 x 4 = 768 KB


def test_a_valid_call_gets_past_the_checks():
    for fn in ENTRIES:
        assert _call(fn=fn) in (0, E_NO_DEVICE)
        assert _call(fn=fn, aprm=False) in (0, E_NO_DEVICE)                                  # NULL: the defaults
        assert _call(fn=fn, p1=0, p2=0, cost_cap=1, paths=4, max_volume_mb=1, ssd_win=0) in (0, E_NO_DEVICE)
        assert _call(fn=fn, p1=4095, p2=4095, cost_cap=4095, paths=8, max_volume_mb=2147483647) in (0, E_NO_DEVICE)
        assert _call(fn=fn, cams=[_cam(), _cam(w=18), _cam(w=18)], off=[0, 1, 1, 3], n_seq=3) in (0, E_NO_DEVICE)
        assert _call(fn=fn, ssd_win=15, ref_frm_count=9, levels=1024, min_refs=8, peak=1.0, ssd_err=0.0, flags=0) in (0, E_NO_DEVICE)


def test_the_file_entries_report_their_errors_before_they_write(tmp_path):
    cams = [[_cam(), _cam()]]
    imgs = [np.zeros((2, 12, 16, 3), np.uint8)]
    d = tmp_path / "seq0"
    d.mkdir()
    for bad_p, bad_a in ((P.depth_recover_params(levels=1), None), (None, P.depth_aggregate_params(paths=5)), (None, P.depth_aggregate_params(p1=200)),
                         (None, P.depth_aggregate_params(cost_cap=0)), (None, P.depth_aggregate_params(max_volume_mb=-2)),
                         (None, P.depth_aggregate_params(reserved=3)), (P.depth_recover_params(reserved=1), None)):
        with pytest.raises(L.MvsError) as e:
            P.RecoverDepthFilesAggregated([str(d)], cams, imgs, bad_p, bad_a)
        assert e.value.code == E_INVALID and "mvs_processor_recover_depths_aggregated:" in str(e.value) and not (d / "DATA").exists()
    with pytest.raises(L.MvsError):
        P.RecoverDepthFilesAggregated([str(d)], cams, [imgs[0][:, :, :8]])
    with pytest.raises(L.MvsError):
        P.RecoverDepthFilesAggregated([str(d), str(d)], cams, imgs)
    with pytest.raises(L.MvsError) as e:                                                 # no frame files: reported with the path, nothing written
        P.RecoverDepthFilesAggregatedFromJpeg([str(d)], cams)
    assert e.value.code == E_IO and "00000.jpg" in str(e.value) and not (d / "DATA").exists()
    lib = L.lib()
    off, arr = L.seq_cams(cams)
    dirs = (C.c_char_p * 1)(os.fsencode(str(d)))
    assert lib.mvs_processor_recover_depths_aggregated(1, dirs, L.ptr(off), arr, None, None, None) == E_INVALID
    assert b"mvs_processor_recover_depths_aggregated:" in lib.mvs_last_error()
    assert lib.mvs_processor_recover_depths_aggregated(1, None, L.ptr(off), arr, L.ptr(imgs[0]), None, None) == E_INVALID
    assert lib.mvs_processor_recover_depths_aggregated(0, dirs, L.ptr(off), arr, L.ptr(imgs[0]), None, None) == E_INVALID
    assert lib.mvs_processor_recover_depths_aggregated_files(1, None, L.ptr(off), arr, None, None) == E_INVALID
    assert b"mvs_processor_recover_depths_aggregated_files:" in lib.mvs_last_error()
    assert lib.mvs_processor_recover_depths_aggregated(1, dirs, L.ptr(off), arr, L.ptr(imgs[0]), None, None) in (0, E_NO_DEVICE)   # NULL: the defaults
    assert not (d / "DATA").exists() or L.device_count() > 0


# ------------------------------------------------------------------ the restatement ----
def test_one_step_of_s2_on_chosen_columns():
    a = A.aparams(p1=3, p2=9)
    prev = np.array([[20], [10], [30], [12]], np.int64)               # M = 10 at level 1
    C = np.array([[1], [2], [3], [4]], np.int64)
    # l = 0: min(20, 10 + 3, 19) = 13; l = 1: 10; l = 2: min(30, 13, 15, 19) = 13; l = 3: min(12, 33, 19) = 12 — each minus M
    assert A._step(C, prev, a).ravel().tolist() == [1 + 3, 2 + 0, 3 + 3, 4 + 2]
    assert A._step(C, prev, A.aparams(p1=0, p2=0)).ravel().tolist() == [1, 2, 3, 4]
    C3 = np.arange(24, dtype=np.int64).reshape(2, 3, 4)
    for dx, dy in A.DIRECTIONS[8]:
        assert np.array_equal(A.path(C3, dx, dy, A.aparams(p1=0, p2=0)), C3)
    one = np.arange(10, dtype=np.int64).reshape(2, 5, 1)              # a rectangle one pixel wide: every path with dx != 0 is one pixel long
    for dx, dy in A.DIRECTIONS[8]:
        if dx != 0:
            assert np.array_equal(A.path(one, dx, dy, A.aparams()), one)


def test_without_penalties_the_call_is_the_winner_takes_all_of_the_capped_cost():
    for paths in (4, 8):
        _, imgs, p = G.scene("A33")
        a = A.aparams(p1=0, p2=0, paths=paths)
        (ref,) = A.aggregate(G.plain("A33"), imgs, p, a)
        for f, fr in enumerate(ref["frames"]):
            assert np.array_equal(fr["S"], paths * fr["C"])
            assert np.array_equal(fr["best"], fr["C"].argmin(axis=0))                       # argmin takes the first: the lower-l rule
            assert np.array_equal(ref["agg"][f][fr["cand"]], paths * fr["C"].min(axis=0).ravel())
            assert fr["C"].max() <= a["cost_cap"] and fr["C"].min() >= 0


@pytest.mark.parametrize("name,variant", G.CASES, ids=[f"{n}-{v}" for n, v in G.CASES])
def test_bounds_outputs_and_scene_conditions(name, variant):
    """L_r <= cost_cap + p2 and S fits uint16; rejected and outside pixels as S4 says; every decision an fp64 operation feeds clears its
    margin, so that a last-bit difference cannot move it; the substep changes out alone"""
    _, imgs, p = G.scene(name)
    a = G.aparams_of(variant)
    on, off = G.reference(name, variant, R.SUBSTEP), G.reference(name, variant, 0)
    for k, (ref, plain) in enumerate(zip(on, off)):
        assert all(np.array_equal(ref[key], plain[key]) for key in ("level", "sum", "cnt", "agg"))
        mg = ref["margins"]
        print(name, variant, k, {kind: f"{v:.2e}" for kind, v in mg.items()}, "accepted", int((ref["level"] >= 0).sum()))
        assert mg.get("coord", 1.0) >= G.MARGIN and mg.get("z", 1.0) >= G.MARGIN
        assert mg.get("accept", 1.0) >= G.MARGIN and mg.get("peak", 1.0) >= G.MARGIN
        assert mg.get("range", 1.0) >= G.RANGE_MARGIN and mg.get("nudge", 1.0) >= G.RANGE_MARGIN
        for r in (ref, plain):
            acc = r["level"] >= 0
            wide = r["out"].astype(np.float64)
            assert ((wide[acc] >= p["dsp_min"]) & (wide[acc] <= p["dsp_max"])).all() and (r["level"][acc] < p["levels"]).all()
            assert (r["out"].view(np.uint32)[~acc] == 0).all() and ((r["sum"] == -1) == (r["cnt"] == 0)).all()
            assert (r["cnt"][acc] >= p["min_refs"]).all()
        for f, fr in enumerate(ref["frames"]):
            if fr["S"] is None:
                continue
            assert fr["Lmax"] <= a["cost_cap"] + a["p2"] and fr["S"].max() <= a["paths"] * (a["cost_cap"] + a["p2"]) <= 65535
            assert (ref["agg"][f][~fr["cand"]] == -1).all() and (ref["agg"][f][fr["cand"]] >= 0).all()
            assert (ref["cnt"][f][~fr["cand"]] == 0).all() and (ref["level"][f][~fr["cand"]] == R.NONE).all()
    accepted = sum(int((r["level"] >= 0).sum()) for r in on)
    if name == "STRIP":
        assert all(fr["C"].shape[1:] == (6, 1) for fr in on[0]["frames"]) and accepted > 5
    if name == "W15":
        assert all(fr["C"].shape[1:] == (6, 10) for fr in on[0]["frames"]) and accepted > 100
    if name in ("A33", "A64", "A65", "A1024", "B33", "AC") and variant != "cap1":
        assert accepted > 300
        assert sum(int((a_["out"] != b_["out"]).sum()) for a_, b_ in zip(on, off)) > 50                    # the substep moves values
    if variant == "cap1":                                             # C is 0 or 1: S ties at most levels and the lowest wins
        lv = np.concatenate([fr["best"].ravel() for fr in on[0]["frames"]])
        assert (lv == 0).mean() > 0.3
    if variant in ("p4", "p8") and name == "A33":                     # aggregation is not a no-op on this scene
        (wta,) = G.reference("A33", "zero")
        assert (wta["level"] != on[0]["level"]).sum() > 0


def test_the_grouping_cannot_matter_to_the_restatement_and_sequences_do_not_see_each_other():
    both = G.reference("AC", "p8")
    (alone,) = A.aggregate([G.plain("AC")[1]], [G.scene("AC")[1][1]], G.scene("AC")[2], G.aparams_of("p8"))
    assert all(np.array_equal(alone[key], both[1][key]) for key in ("out", "level", "sum", "cnt", "agg"))


def test_the_recorded_quality():
    """measured on the restatements alone; tests/depth_sgm_scenes.py records the run and what was tried"""
    for name in ("A33", "A33n"):
        q, want = G.quality_of(name), G.QUALITY[name]
        print(name, q, "recorded", want)
        assert q == want
        # what is required of the restatement at the default penalties
        assert q["aggregated"]["within"] >= q["plain"]["within"] and q["aggregated"]["beyond"] <= q["plain"]["beyond"]


def test_the_recorded_amplitudes_and_penalties():
    """the reason for staying at amplitude 4 and for the defaults, run again: the plain sweep's (accepted, beyond) at every amplitude, and
    the aggregated (accepted, within, beyond) of every triple that was tried"""
    got = {amp: (q["accepted"], q["beyond"]) for amp, q in ((amp, G.plain_quality(amp)) for amp in G.AMPLITUDES)}
    print(got)
    assert got == G.AMPLITUDES and set(G.AMPLITUDES) == {0, 4, 8, 16, 32}
    assert not any(got[amp][1] >= 2 * got[0][1] for amp in (4, 8, 16, 32))                # no amplitude doubles the plain sweep's gross errors
    assert G.NOISE_AMP == 4
    for (p1, p2, cap), (noisy, clean) in G.PENALTIES.items():
        for amp, want in ((G.NOISE_AMP, noisy), (0, clean)):
            if want is not None:
                q = G.aggregated_quality(amp, A.aparams(p1=p1, p2=p2, cost_cap=cap))
                assert (q["accepted"], q["within"], q["beyond"]) == want, ((p1, p2, cap), amp, q, want)
    a = A.aparams()
    assert G.PENALTIES[(a["p1"], a["p2"], a["cost_cap"])] == ((3780, 3780, 0), (3825, 3824, 1)) and (64, 1024, 4095) in G.PENALTIES


# ------------------------------------------------------------------ the shared rules ----
def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "depth_sgm_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "depth_sgm_rules.cpp"), "-o", exe])
    return exe


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """tests/depth_sgm_rules.cpp: S1's division and cap, each term of S2, S4-S6 on chosen numbers; then S1-S6 of the header (sg_frame, a
    plain loop per rule over heap blocks of exact size) on A33 and STRIP against the restatement, paths 4 and 8, with and without the
    substep: level, sum, cnt and agg exactly, out bit for bit (host code, no contraction)"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "depth sgm rules ok" in run.stdout, run.stdout + run.stderr
    for name, variant, flags in (("A33", "p8", R.SUBSTEP), ("A33", "p4", 0), ("A33", "equal", R.SUBSTEP), ("STRIP", "p8", R.SUBSTEP), ("STRIP", "p4", 0)):
        (cams,), (imgs,), p = G.scene(name)
        a = G.aparams_of(variant)
        n, h, w = imgs.shape[:3]
        (ref,) = G.reference(name, variant, flags)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as fh:
            fh.write(np.asarray([n, w, h, p["ssd_win"], p["ref_frm_count"], p["levels"], p["min_refs"], flags, a["p1"], a["p2"], a["cost_cap"],
                                 a["paths"]], np.int32).tobytes())
            fh.write(np.asarray([p["dsp_min"], p["dsp_max"], p["ssd_err"], p["peak"]], np.float64).tobytes())
            for c in cams:
                fh.write(np.concatenate([[c.fx, c.fy, c.cx, c.cy], np.asarray(c.R, np.float64).reshape(9), np.asarray(c.t, np.float64).reshape(3)]).tobytes())
            fh.write(imgs.tobytes())
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = open(fout, "rb").read()
        m = n * h * w
        assert len(raw) == 15 * m
        out = np.frombuffer(raw[:4 * m], np.uint32).reshape(n, h, w)
        sm = np.frombuffer(raw[4 * m:8 * m], np.int32).reshape(n, h, w)
        ag = np.frombuffer(raw[8 * m:12 * m], np.int32).reshape(n, h, w)
        lv = np.frombuffer(raw[12 * m:14 * m], np.int16).reshape(n, h, w)
        cnt = np.frombuffer(raw[14 * m:], np.uint8).reshape(n, h, w)
        assert np.array_equal(lv, ref["level"]) and np.array_equal(sm, ref["sum"]) and np.array_equal(cnt, ref["cnt"]) and np.array_equal(ag, ref["agg"])
        assert np.array_equal(out, ref["out"].view(np.uint32))
