"""mvs_point_sample on the GPU (csrc/pointsample.hip) against the numpy restatement tests/ref_pointsample.py on the six scenes of
tests/pointsample_scenes.py: the candidate table of rule 6 and the emitted (frame, pixel) lists exactly — every decision of these scenes
clears 1e-9 (tests/test_pointsample_host.py), so a last-bit difference cannot move one —, points and normals within 1e-12; batching, the
device form, run-to-run identity, capacity, the optional outputs, the chain CheckConsistency -> RunPointSample -> StitchPointSets and the
file entry."""
import ctypes as C

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P, scene as S
from tests import pointsample_scenes as SC

pytestmark = pytest.mark.gpu
TOL = 1e-12


def tables(cameras):
    off = np.zeros(len(cameras) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in cameras])
    flat = [L.CCamera.of(c) for seq in cameras for c in seq]
    return off, (L.CCamera * len(flat))(*flat), len(flat)


def gpu_candidates(cameras, depths, p):
    off, cams, ncam = tables(cameras)
    flat = np.concatenate([d.reshape(-1) for d in depths])
    coff = np.zeros(ncam + 1, np.int64)
    prm = SC.c_params(p)
    cap = sum(len(c) * (-(-c[0].w // p["pt_samp_rds"])) * (-(-c[0].h // p["pt_samp_rds"])) for c in cameras)
    cand = np.full(cap, -7, np.int32)
    L.check(L.lib().mvs_test_point_sample_candidates(len(cameras), L.ptr(off), cams, L.ptr(flat), C.byref(prm), L.ptr(coff), L.ptr(cand), cap))
    assert coff[-1] == cap
    return coff, cand


def raw_call(cameras, depths, p, cap, frame=True, pixel=True):
    off, cams, _ = tables(cameras)
    flat = np.concatenate([d.reshape(-1) for d in depths])
    soff = np.full(len(cameras) + 1, -1, np.int64)
    pts, nrm = np.full((max(cap, 1), 3), np.nan), np.full((max(cap, 1), 3), np.nan)
    frm, pix = (np.full(max(cap, 1), -1, np.int32) if frame else None), (np.full(max(cap, 1), -1, np.int32) if pixel else None)
    prm = SC.c_params(p)
    rc = L.lib().mvs_point_sample(len(cameras), L.ptr(off), cams, L.ptr(flat), C.byref(prm), L.ptr(soff), L.ptr(pts), L.ptr(nrm), L.ptr(frm), L.ptr(pix), cap)
    return rc, soff, pts, nrm, frm, pix


@pytest.mark.parametrize("name", SC.NAMES)
def test_candidates_and_emitted_lists_equal_the_restatement(name):
    cameras, depths, p = SC.scene(name)
    ref = SC.reference(name)
    coff, cand = gpu_candidates(cameras, depths, p)
    want = np.concatenate([r["cand"].reshape(-1) for r in ref])
    differ = np.flatnonzero(cand != want)
    assert len(differ) == 0, (name, "candidate cells that differ", differ[:8], cand[differ[:8]], want[differ[:8]])
    cam = 0
    for cams, r in zip(cameras, ref):                                  # the offsets bracket every camera's frame
        for f in range(len(cams)):
            assert coff[cam + 1] - coff[cam] == r["cand"].shape[1]
            cam += 1
    got = P.RunPointSample(cameras, depths, SC.c_params(p))
    for k, (r, (pts, nrm, frm, pix)) in enumerate(zip(ref, got)):
        assert np.array_equal(frm, r["frame"]) and np.array_equal(pix, r["pixel"]), (name, k, len(pix), len(r["pixel"]))
        ep, en = float(np.abs(pts - r["points"]).max()), float(np.abs(nrm - r["normals"]).max())
        print(f"{name}[{k}]: {len(pix)} points; max |point difference| {ep:.2e}, max |normal difference| {en:.2e} (bound {TOL:.0e})")
        assert ep <= TOL and en <= TOL


def test_the_host_callable_camera_maps_are_the_device_ones():
    """camera_dev.h keeps world_from_img / img_from_world as __device__ inlines and adds __host__ __device__ copies for the shared rules.
    The kernels that run the former tie them to the latter: mvs_depth_unproject's point of every emitted pixel is mvs_point_sample's, bit
    for bit, and mvs_visibility_cull keeps exactly the emitted points that land inside every frame by the restatement's projection
    (which the shared rules equal, test above)."""
    from multiviewstitch_amd import srt
    from tests import ref_pointsample as R
    cameras, depths, p = SC.scene("A")
    (cams,), (dsp,) = cameras, depths
    ((pts, nrm, frm, pix),) = P.RunPointSample(cameras, depths, SC.c_params(p))
    for f in range(len(cams)):
        dense, valid = srt.depth_unproject(dsp[f], cams[f], p["dsp_min"], p["dsp_max"])
        sel = frm == f
        assert valid[pix[sel]].all() and dense[pix[sel]].tobytes() == pts[sel].tobytes()
    import dataclasses
    crop = [dataclasses.replace(c, w=60, h=40) for c in cams]          # the top-left 60 x 40 of every frame: part of the points fall outside
    keep, _ = srt.visibility_cull(pts, [1.0], [np.eye(3)], [np.zeros(3)], [crop])
    inside = np.ones(len(pts), bool)
    for c in crop:
        inside &= R.agrees(tuple(pts[:, i] for i in range(3)), c, np.zeros((40, 60), np.float32), p, R.Margins())[3]
    assert 0 < inside.sum() < len(pts) and np.array_equal(keep.astype(bool), inside)


def test_one_flat_tensor_is_read_in_place_on_a_stream_that_is_not_current():
    import torch
    cameras, depths, p = SC.scene("AB")
    host = P.RunPointSample(cameras, depths, SC.c_params(p))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        flat = torch.from_numpy(np.concatenate([d.reshape(-1) for d in depths])).cuda()
        lists = [torch.from_numpy(np.array(d)).cuda() for d in depths]
    assert torch.cuda.current_stream() != st                            # the rasters are pending on st; the call must order itself there
    for arg in (flat, lists):
        dev = P.RunPointSample(cameras, arg, SC.c_params(p), stream=st.cuda_stream)
        for x, y in zip(host, dev):
            assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(x, y))


def test_two_sequences_in_one_call_equal_two_calls():
    cameras, depths, p = SC.scene("AB")
    both = P.RunPointSample(cameras, depths, SC.c_params(p))
    for k in range(2):
        (alone,) = P.RunPointSample([cameras[k]], [depths[k]], SC.c_params(p))
        assert len(alone[0]) > 100
        for a, b in zip(alone, both[k]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_an_empty_sequence_between_two_emits_nothing():
    cameras, depths, p = SC.scene("AB")
    got = P.RunPointSample([cameras[0], [], cameras[1]], [depths[0], np.zeros((0, 4, 4), np.float32), depths[1]], SC.c_params(p))
    want = P.RunPointSample(cameras, depths, SC.c_params(p))
    assert len(got[1][0]) == 0 and all(a.tobytes() == b.tobytes() for k, j in ((0, 0), (2, 1)) for a, b in zip(got[k], want[j]))


def test_the_device_form_on_a_stream_equals_the_host_form_and_runs_are_identical():
    import torch
    cameras, depths, p = SC.scene("AB")
    host = P.RunPointSample(cameras, depths, SC.c_params(p))
    again = P.RunPointSample(cameras, depths, SC.c_params(p))
    assert all(a.tobytes() == b.tobytes() for x, y in zip(host, again) for a, b in zip(x, y))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dd = [torch.from_numpy(np.array(d)).cuda() for d in depths]
        st.synchronize()
        for capacity in (None, 3):                                      # 3: the first attempt is too small and the call is repeated
            dev = P.RunPointSample(cameras, dd, SC.c_params(p), stream=st.cuda_stream, capacity=capacity)
            for x, y in zip(host, dev):
                assert all(t.is_cuda for t in y) and len(x[0]) == len(y[0])
                assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(x, y))


def test_a_capacity_that_is_too_small_reports_the_need():
    cameras, depths, p = SC.scene("AB")
    ref = SC.reference("AB")
    need = [len(r["pixel"]) for r in ref]
    rc, soff, pts, _, _, _ = raw_call(cameras, depths, p, sum(need) - 1)
    assert rc == -1 and b"capacity" in L.lib().mvs_last_error()
    assert soff.tolist() == [0, need[0], need[0] + need[1]] and np.isnan(pts).all()       # nothing was written
    rc, soff, pts, _, _, _ = raw_call(cameras, depths, p, 0)
    assert rc == -1 and soff[-1] == sum(need)
    rc, soff, pts, nrm, frm, pix = raw_call(cameras, depths, p, sum(need))
    assert rc == 0 and not np.isnan(pts).any() and not np.isnan(nrm).any()


def test_frame_and_pixel_may_be_null():
    cameras, depths, p = SC.scene("B")
    (ref,) = SC.reference("B")
    cap = len(ref["pixel"])
    full = raw_call(cameras, depths, p, cap)
    for frame, pixel in ((False, True), (True, False), (False, False)):
        rc, soff, pts, nrm, frm, pix = raw_call(cameras, depths, p, cap, frame, pixel)
        assert rc == 0 and soff[-1] == cap and pts.tobytes() == full[2].tobytes() and nrm.tobytes() == full[3].tobytes()
        assert frm is None or np.array_equal(frm, ref["frame"])
        assert pix is None or np.array_equal(pix, ref["pixel"])


def test_chain_check_consistency_point_sample_stitch(tmp_path):
    """scene AB: CheckConsistency's rasters -> RunPointSample -> mvs_npts_write -> StitchPointSets with the identity SRT; PSR.npts holds the
    rows the stitch keeps of what it read"""
    from tests import ref_stitch as RS
    cameras, depths, p = SC.scene("AB")
    checked = [P.CheckConsistency(c, d, S.MIN_DSP, S.MAX_DSP, 2) for c, d in zip(cameras, depths)]
    assert all(300 < (c != 0).sum() <= (d != 0).sum() for c, d in zip(checked, depths))
    got = P.RunPointSample(cameras, checked, SC.c_params(p))
    paths = []
    for k, (pts, nrm, frm, pix) in enumerate(got):
        assert len(pts) > 50 and (np.diff(frm.astype(np.int64) * 2 ** 31 + pix) > 0).all()
        paths.append(str(tmp_path / f"seq{k}.npts"))
        IO.write_npts(paths[-1], pts, nrm)
    res = tmp_path / "Result"
    res.mkdir()
    scales, Rs, ts = np.ones(2), np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
    nk = P.StitchPointSets(paths, scales, Rs, ts, cameras, str(res), truncate=True)
    rp, rn = zip(*[IO.read_npts(q) for q in paths])
    out, nk_ref = RS.stitch(list(rp), list(rn), scales, Rs, ts, cameras, truncate=True)
    assert np.array_equal(nk, nk_ref) and nk.sum() > 100
    got_bytes = (res / "PSR.npts").read_bytes()
    IO.write_npts(str(res / "PSR.npts"), np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]))
    assert got_bytes == (res / "PSR.npts").read_bytes()


def test_the_file_entry_writes_what_run_point_sample_returns(tmp_path):
    cameras, depths, p = SC.scene("AB")
    dirs = []
    for k, d in enumerate(depths):
        dirs.append(str(tmp_path / f"seq{k}"))
        (tmp_path / f"seq{k}" / "DATA" / "CHECK").mkdir(parents=True)
        for i, ras in enumerate(d):
            IO.SaveDepth(str(tmp_path / f"seq{k}" / "DATA" / "CHECK" / f"_depth{i}.raw"), ras)
    cnt = P.PointSampleFiles(dirs, cameras, SC.c_params(p))
    got = P.RunPointSample(cameras, depths, SC.c_params(p))
    for k, (pts, nrm, _, _) in enumerate(got):
        assert cnt[k] == len(pts)
        want = tmp_path / f"want{k}.npts"
        IO.write_npts(str(want), pts, nrm)                             # float32 / %g
        assert (tmp_path / f"seq{k}" / "Rec" / "PointSample.npts").read_bytes() == want.read_bytes()
    other = str(tmp_path / "elsewhere.npts")
    P.PointSampleFiles(dirs[:1], cameras[:1], SC.c_params(p), npts_paths=[other])
    assert open(other, "rb").read() == (tmp_path / "want0.npts").read_bytes()
