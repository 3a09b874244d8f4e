"""mvs_refine_depth_maps on the GPU (csrc/depth_refine.hip) against the numpy restatement tests/ref_depth_refine.py on the scenes of
tests/depth_refine_scenes.py: k_out, sum_out and cnt_out exactly — every decision of these scenes clears its margin
(tests/test_depth_refine_host.py), so a last-bit difference cannot move one —, out bit for bit without the substep and within one float32
ulp with it; pass-through, the optional outputs, the device form, batching, run-to-run identity, the properties of one-frame, one-colour and
one-window calls, the chain RenderViews -> RefineAllDepthMaps -> CheckConsistency -> RunPointSample and the file entry."""
import ctypes as C

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P, scene as S
from tests import depth_refine_scenes as SC, ref_depth_refine as R

pytestmark = pytest.mark.gpu


def run(name, flags, **kw):
    cameras, imgs, depths, p = SC.scene(name)
    return P.RefineAllDepthMaps(cameras, imgs, depths, SC.c_params(p, flags=flags), with_detail=True, **kw)


def ulps(a, b):
    """distance in float32 steps between two arrays of finite floats of one sign"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("flags", (0, R.SUBSTEP), ids=("plain", "substep"))
@pytest.mark.parametrize("name", SC.NAMES)
def test_every_output_equals_the_restatement(name, flags):
    _, _, depths, _ = SC.scene(name)
    for k, (dsp, ref, (out, kk, sm, cnt)) in enumerate(zip(depths, SC.reference(name, flags), run(name, flags))):
        assert out.dtype == np.float32 and kk.dtype == np.int8 and sm.dtype == np.int32 and cnt.dtype == np.uint8 and out.shape == dsp.shape
        for what, got, want in (("k", kk, ref["k"]), ("sum", sm, ref["sum"]), ("cnt", cnt, ref["cnt"])):
            differ = np.argwhere(got != want)
            assert len(differ) == 0, (name, k, what, len(differ), differ[:4].tolist(), got[got != want][:4], want[got != want][:4])
        keep = kk == R.NONE                                         # non-candidates and rejected pixels: the input, bit for bit
        assert np.array_equal(out.view(np.uint32)[keep], dsp.view(np.uint32)[keep])
        bits = int((out.view(np.uint32) != ref["out"].view(np.uint32)).sum())
        print(f"{name}[{k}] flags {flags}: {int((~keep).sum())} accepted pixels, {bits} whose out differs from the restatement in any bit")
        if flags == 0:
            assert bits == 0
        else:
            assert int(ulps(out[~keep], ref["out"][~keep]).max(initial=0)) <= 1
            assert bits == 0                                        # expected: every operation is an IEEE fp64 one in the stated order


def test_the_optional_outputs_may_be_null():
    cameras, imgs, depths, p = SC.scene("AC")
    full = P.RefineAllDepthMaps(cameras, imgs, depths, SC.c_params(p), with_detail=True)
    bare = P.RefineAllDepthMaps(cameras, imgs, depths, SC.c_params(p))
    assert all(a.tobytes() == b[0].tobytes() for a, b in zip(bare, full))
    off, cams = L.seq_cams(cameras)
    fi, fd = np.concatenate([i.reshape(-1) for i in imgs]), np.concatenate([d.reshape(-1) for d in depths])
    want = np.concatenate([b[0].reshape(-1) for b in full])
    prm = SC.c_params(p)
    for which in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):
        out = np.zeros(len(fd), np.float32)
        opt = [np.zeros(len(fd), dt) if on else None for on, dt in zip(which, (np.int8, np.int32, np.uint8))]
        L.check(L.lib().mvs_refine_depth_maps(len(cameras), L.ptr(off), cams, L.ptr(fi), L.ptr(fd), C.byref(prm), L.ptr(out), *[L.ptr(a) for a in opt]))
        assert out.tobytes() == want.tobytes()
        for j, a in enumerate(opt):
            assert a is None or a.tobytes() == np.concatenate([b[1 + j].reshape(-1) for b in full]).tobytes()


def test_two_sequences_in_one_call_equal_two_calls_and_runs_are_identical():
    cameras, imgs, depths, p = SC.scene("AC")
    both = P.RefineAllDepthMaps(cameras, imgs, depths, SC.c_params(p), with_detail=True)
    again = P.RefineAllDepthMaps(cameras, imgs, depths, SC.c_params(p), with_detail=True)
    assert all(a.tobytes() == b.tobytes() for x, y in zip(both, again) for a, b in zip(x, y))
    for k in range(2):
        (alone,) = P.RefineAllDepthMaps([cameras[k]], [imgs[k]], [depths[k]], SC.c_params(p), with_detail=True)
        assert (alone[1] != R.NONE).sum() > 300
        for a, b in zip(alone, both[k]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    got = P.RefineAllDepthMaps([cameras[0], [], cameras[1]], [imgs[0], np.zeros((0, 4, 4, 3), np.uint8), imgs[1]],
                               [depths[0], np.zeros((0, 4, 4), np.float32), depths[1]], SC.c_params(p), with_detail=True)
    assert got[1][0].size == 0 and all(a.tobytes() == b.tobytes() for i, j in ((0, 0), (2, 1)) for a, b in zip(got[i], both[j]))


def test_the_device_form_on_a_stream_equals_the_host_form():
    import torch
    cameras, imgs, depths, p = SC.scene("AC")
    host = P.RefineAllDepthMaps(cameras, imgs, depths, SC.c_params(p), with_detail=True)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        di = [torch.from_numpy(np.array(i)).cuda() for i in imgs]
        dd = [torch.from_numpy(np.array(d)).cuda() for d in depths]
    assert torch.cuda.current_stream() != st                        # the inputs are pending on st; the call must order itself there
    dev = P.RefineAllDepthMaps(cameras, di, dd, SC.c_params(p), stream=st.cuda_stream, with_detail=True)
    for x, y in zip(host, dev):
        assert all(t.is_cuda for t in y)
        assert all(a.dtype == b.cpu().numpy().dtype and a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(x, y))
    bare = P.RefineAllDepthMaps(cameras, di, dd, SC.c_params(p), stream=st.cuda_stream)
    assert all(a[0].tobytes() == b.cpu().numpy().tobytes() for a, b in zip(host, bare))


def test_one_frame_one_window_and_one_colour():
    for name in ("D", "E_R1"):
        _, _, depths, _ = SC.scene(name)
        for dsp, (out, kk, sm, cnt) in zip(depths, run(name, R.SUBSTEP)):
            assert out.tobytes() == dsp.tobytes() and (kk == R.NONE).all() and (sm == -1).all() and (cnt == 0).all()
    cameras, imgs, depths, p = SC.scene("A")
    flat = [np.full_like(i, 77) for i in imgs]
    for flags in (0, R.SUBSTEP):
        ((out, kk, sm, cnt),) = P.RefineAllDepthMaps(cameras, flat, depths, SC.c_params(p, flags=flags), with_detail=True)
        (ref,) = R.refine(cameras, flat, depths, dict(p, flags=flags))
        zero, other = SC.one_colour_expectation(ref, depths[0], p["steps"])
        assert zero > 1000 and np.array_equal(kk, ref["k"]) and np.array_equal(sm, ref["sum"]) and np.array_equal(cnt, ref["cnt"])
        assert out.tobytes() == ref["out"].tobytes()
        assert (out.view(np.uint32) == depths[0].view(np.uint32))[(kk == 0) | (kk == R.NONE)].all() and (sm[cnt > 0] == 0).all()


def test_chain_render_refine_check_point_sample():
    """a small mesh (the geodesic sphere) rendered into the cameras of scene A's rig, refined against images of that sphere, checked and
    sampled: the refined rasters are what CheckConsistency and RunPointSample read"""
    cams, _, _, _, _ = SC._sequence("A")
    verts, faces = S.geodesic_sphere(8)
    verts = 0.25 * verts
    ras = P.RenderViews(verts, faces, [cams])
    assert ras.shape == (len(cams), cams[0].h, cams[0].w) and (ras > 0).sum() > 1000
    imgs = np.zeros(ras.shape + (3,), np.uint8)
    for f, c in enumerate(cams):                                    # texture at the rendered surface point of every covered pixel
        Rm, t = np.asarray(c.R), np.asarray(c.t)
        vv, uu = np.mgrid[0:c.h, 0:c.w].astype(np.float64)
        z = 1.0 / np.where(ras[f] > 0, ras[f], 1.0).astype(np.float64)
        X = (np.stack([(uu - c.cx) * z / c.fx, (vv - c.cy) * z / c.fy, z], -1) - t) @ Rm
        imgs[f] = np.where((ras[f] > 0)[..., None], SC.texture(X, 21), 0)
    prm = P.depth_refine_params(dsp_min=SC.DSP_MIN, dsp_max=SC.DSP_MAX, rel_range=0.02, ssd_win=3, steps=4, ssd_err=40.0)
    (refined, kk, _, _), = P.RefineAllDepthMaps([cams], [imgs], [ras], prm, with_detail=True)
    assert (kk != R.NONE).sum() > 500 and np.array_equal(refined == 0, ras == 0)
    assert np.abs(refined[kk != R.NONE] / ras[kk != R.NONE] - 1.0).max() <= 0.02 * (1 + 0.5 / 4) + 1e-6
    checked = P.CheckConsistency(cams, refined, SC.DSP_MIN, SC.DSP_MAX, 2)
    assert (checked != 0).sum() > 500
    ((pts, nrm, frm, pix),) = P.RunPointSample([cams], [checked], P.point_sample_params(dsp_min=SC.DSP_MIN, dsp_max=SC.DSP_MAX, max_dsp_err=0.01))
    assert len(pts) > 50 and np.abs(np.sqrt((pts * pts).sum(1)) - 0.25).max() < 0.1      # 2 % of a depth of 3, and the facets


def test_the_file_entry_writes_what_the_call_returns(tmp_path):
    cameras, imgs, depths, p = SC.scene("AC")
    dirs = []
    for k, d in enumerate(depths):
        dirs.append(str(tmp_path / f"seq{k}"))
        (tmp_path / f"seq{k}" / "DATA" / "Render").mkdir(parents=True)
        for i, ras in enumerate(d):
            IO.SaveDepth(str(tmp_path / f"seq{k}" / "DATA" / "Render" / f"_depth{i}.raw"), ras)
    P.RefineDepthFiles(dirs, cameras, imgs, SC.c_params(p))
    got = P.RefineAllDepthMaps(cameras, imgs, depths, SC.c_params(p))
    for k, (cams, out) in enumerate(zip(cameras, got)):
        for i, c in enumerate(cams):
            back = np.empty((c.h, c.w), np.float32)
            L.check(L.lib().mvs_depth_raw_read(str(tmp_path / f"seq{k}" / "DATA" / "Refine" / f"_depth{i}.raw").encode(), c.w, c.h, L.ptr(back)))
            assert back.tobytes() == out[i].tobytes()
        assert not (tmp_path / f"seq{k}" / "DATA" / "Refine" / f"_depth{len(cams)}.raw").exists()
