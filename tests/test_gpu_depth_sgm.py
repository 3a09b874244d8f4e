"""mvs_recover_depth_maps_aggregated on the GPU (csrc/depth_sgm.hip) against the numpy restatement tests/ref_depth_sgm.py on the scenes
and variants of tests/depth_sgm_scenes.py: level_out, sum_out, cnt_out and agg_out exactly, out bit for bit with and without the substep
— every decision of these scenes clears its margin (tests/test_depth_sgm_host.py), and everything between the raw sums and the winner is
integers —; rejected and outside pixels, the optional outputs, the device form on a stream, the grouping of frames, run-to-run identity,
the file entries, and the chain into CheckConsistency and RunPointSample."""
import ctypes as C
import itertools

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import depth_sgm_scenes as G, ref_depth_recover as R

pytestmark = pytest.mark.gpu


def run(name, variant, flags=R.SUBSTEP, **kw):
    cameras, imgs, p = G.scene(name)
    return P.RecoverDepthMapsAggregated(cameras, imgs, G.c_params(p, flags=flags), G.c_aparams(variant, **kw), with_detail=True)


def same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for s, t in zip(a, b) for x, y in zip(s, t))


@pytest.mark.parametrize("flags", (0, R.SUBSTEP), ids=("plain", "substep"))
@pytest.mark.parametrize("name,variant", G.CASES, ids=[f"{n}-{v}" for n, v in G.CASES])
def test_every_output_equals_the_restatement(name, variant, flags):
    _, imgs, _ = G.scene(name)
    for k, (img, ref, got) in enumerate(zip(imgs, G.reference(name, variant, flags), run(name, variant, flags))):
        out, lv, sm, cnt, agg = got
        assert [a.dtype for a in got] == [np.float32, np.int16, np.int32, np.uint8, np.int32] and all(a.shape == img.shape[:3] for a in got)
        for what, have, want in (("agg", agg, ref["agg"]), ("sum", sm, ref["sum"]), ("cnt", cnt, ref["cnt"]), ("level", lv, ref["level"])):
            differ = np.argwhere(have != want)
            print(f"{name}-{variant}[{k}] flags {flags} {what}: {len(differ)} entries differ")
            assert len(differ) == 0, (name, variant, k, what, len(differ), differ[:4].tolist(), have[have != want][:4], want[have != want][:4])
        bits = int((out.view(np.uint32) != ref["out"].view(np.uint32)).sum())
        print(f"{name}-{variant}[{k}] flags {flags}: {int((lv >= 0).sum())} accepted pixels, {bits} whose out differs from the restatement in any bit")
        assert bits == 0
        # S4: rejected and outside pixels
        none = lv == R.NONE
        assert (out.view(np.uint32)[none] == 0).all()
        for f, fr in enumerate(ref["frames"]):
            outside = ~fr["cand"]
            assert (lv[f][outside] == -1).all() and (sm[f][outside] == -1).all() and (cnt[f][outside] == 0).all() and (agg[f][outside] == -1).all()
            assert (agg[f][fr["cand"]] >= 0).all()
        assert ((sm == -1) == (cnt == 0)).all() and (lv[cnt == 0] == -1).all()


def test_accepted_values_lie_in_the_range():
    for name in ("A33", "B33", "A1024"):
        _, _, p = G.scene(name)
        for out, lv, _, _, _ in run(name, "p8"):
            wide = out[lv >= 0].astype(np.float64)
            assert len(wide) > 300 and ((wide >= p["dsp_min"]) & (wide <= p["dsp_max"])).all() and np.array_equal(out != 0, lv >= 0)


def test_the_optional_outputs_may_be_null():
    cameras, imgs, p = G.scene("AC")
    full = run("AC", "p8")
    bare = P.RecoverDepthMapsAggregated(cameras, imgs, G.c_params(p), G.c_aparams("p8"))
    assert all(a.tobytes() == b[0].tobytes() for a, b in zip(bare, full))
    off, cams = L.seq_cams(cameras)
    fi = np.concatenate([i.reshape(-1) for i in imgs])
    want = [np.concatenate([b[j].reshape(-1) for b in full]) for j in range(5)]
    prm, aprm = G.c_params(p), G.c_aparams("p8")
    for which in itertools.product((0, 1), repeat=4):
        out = np.ones(len(want[0]), np.float32)
        opt = [np.zeros(len(out), dt) if on else None for on, dt in zip(which, (np.int16, np.int32, np.uint8, np.int32))]
        L.check(L.lib().mvs_recover_depth_maps_aggregated(len(cameras), L.ptr(off), cams, L.ptr(fi), C.byref(prm), C.byref(aprm), L.ptr(out),
                                                          *[L.ptr(a) for a in opt]))
        assert out.tobytes() == want[0].tobytes()
        for j, a in enumerate(opt):
            assert a is None or a.tobytes() == want[1 + j].tobytes()
    out = np.ones(len(want[0]), np.float32)                             # NULL aggregation parameters are the defaults, which p8 is
    L.check(L.lib().mvs_recover_depth_maps_aggregated(len(cameras), L.ptr(off), cams, L.ptr(fi), C.byref(prm), None, L.ptr(out), None, None, None, None))
    assert out.tobytes() == want[0].tobytes()


def test_the_device_form_on_a_stream_equals_the_host_form():
    import torch
    cameras, imgs, p = G.scene("AC")
    host = run("AC", "p8")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        di = [torch.from_numpy(np.array(i)).cuda() for i in imgs]
    assert torch.cuda.current_stream() != st                        # the inputs are pending on st; the call must order itself there
    dev = P.RecoverDepthMapsAggregated(cameras, di, G.c_params(p), G.c_aparams("p8"), stream=st.cuda_stream, with_detail=True)
    for x, y in zip(host, dev):
        assert all(t.is_cuda for t in y)
        assert all(a.dtype == b.cpu().numpy().dtype and a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(x, y))
    bare = P.RecoverDepthMapsAggregated(cameras, di, G.c_params(p), G.c_aparams("p8"), stream=st.cuda_stream)
    assert all(a[0].tobytes() == b.cpu().numpy().tobytes() for a, b in zip(host, bare))


def test_the_grouping_of_frames_changes_no_byte():
    """AC: two sequences in one call against two calls, and two consecutive runs.  Then AC at 320 levels, where the volumes of one frame
    of A (31 x 23 pixels x 320 levels x 4 bytes = 912640) fit max_volume_mb = 1, the smallest budget there is, and those of two do not:
    every frame of A is a group of its own, the two frames of C (19 x 17: 413440 bytes each) share one — against the default budget,
    which holds all eight"""
    cameras, imgs, p = G.scene("AC")
    both, again = run("AC", "p8"), run("AC", "p8")
    assert same(both, again)
    assert sum(int((b[1] >= 0).sum()) for b in both) > 1000
    for k in range(2):
        (alone,) = P.RecoverDepthMapsAggregated([cameras[k]], [imgs[k]], G.c_params(p), G.c_aparams("p8"), with_detail=True)
        assert same([alone], [both[k]])
    assert 4 * 31 * 23 * 320 <= 1 << 20 < 2 * 4 * 31 * 23 * 320 and 2 * 4 * 19 * 17 * 320 <= 1 << 20
    wholes = {}
    for variant in ("p8", "p4"):
        whole = wholes[variant] = P.RecoverDepthMapsAggregated(cameras, imgs, G.c_params(p, levels=320), G.c_aparams(variant), with_detail=True)
        cut = P.RecoverDepthMapsAggregated(cameras, imgs, G.c_params(p, levels=320), G.c_aparams(variant, max_volume_mb=1), with_detail=True)
        assert same(cut, whole) and sum(int((b[1] >= 0).sum()) for b in whole) > 1000
    got = P.RecoverDepthMapsAggregated([cameras[0], [], cameras[1]], [imgs[0], np.zeros((0, 4, 4, 3), np.uint8), imgs[1]], G.c_params(p, levels=320),
                                       G.c_aparams("p8", max_volume_mb=1), with_detail=True)
    assert got[1][0].size == 0 and same([got[0], got[2]], wholes["p8"])


def test_the_file_entries_write_what_the_call_returns(tmp_path):
    cameras, imgs, p = G.scene("AC")
    dirs = [str(tmp_path / f"seq{k}") for k in range(len(cameras))]
    prm, aprm = G.c_params(p), G.c_aparams("p8")
    P.RecoverDepthFilesAggregated(dirs, cameras, imgs, prm, aprm)
    got = P.RecoverDepthMapsAggregated(cameras, imgs, prm, aprm)

    def holds(dirs, got):
        for k, (cams, out) in enumerate(zip(cameras, got)):
            for i, c in enumerate(cams):
                back = np.empty((c.h, c.w), np.float32)
                L.check(L.lib().mvs_depth_raw_read(str(tmp_path / dirs[k] / "DATA" / f"_depth{i}.raw").encode(), c.w, c.h, L.ptr(back)))
                assert back.tobytes() == out[i].tobytes()
            assert not (tmp_path / dirs[k] / "DATA" / f"_depth{len(cams)}.raw").exists()
    holds(dirs, got)
    assert sum(int((g != 0).sum()) for g in got) > 1000
    jdirs, back = [str(tmp_path / f"jpg{k}") for k in range(len(cameras))], []
    for d, im in zip(jdirs, imgs):
        (tmp_path / d).mkdir()
        streams = P.EncodeJpegs(im, quality=95, sampling="444", order="RGB")
        for i, s in enumerate(streams):
            (tmp_path / d / f"{i:05d}.jpg").write_bytes(s)
        back.append(P.DecodeJpegs(streams, order="RGB"))
    P.RecoverDepthFilesAggregatedFromJpeg(jdirs, cameras, prm, aprm)
    holds(jdirs, P.RecoverDepthMapsAggregated(cameras, back, prm, aprm))


def test_chain_recover_check_point_sample():
    """scene A's rasters are what CheckConsistency and RunPointSample read: more than a few points come out"""
    (cams,), (imgs,), p = G.scene("A33")
    (rec,) = P.RecoverDepthMapsAggregated([cams], [imgs], G.c_params(p), G.c_aparams("p8"))
    assert (rec != 0).sum() > 3000
    checked = P.CheckConsistency(cams, rec, p["dsp_min"], p["dsp_max"], 2)
    assert (checked != 0).sum() > 500
    ((pts, nrm, frm, pix),) = P.RunPointSample([cams], [checked], P.point_sample_params(dsp_min=p["dsp_min"], dsp_max=p["dsp_max"], max_dsp_err=0.01))
    assert len(pts) > 50 and np.isfinite(pts).all()
