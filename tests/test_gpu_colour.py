"""mvs_colour_vertices on the GPU against the numpy restatement tests/ref_colour.py: colours and counts byte for byte on every vertex of
every scene of tests/colour_scenes.py (tests/test_colour_host.py::test_scene_conditions is why no vertex has to be set aside), with both
kernel mappings; the device form on a stream; scene O on rasters the GPU rendered itself; and the file form."""
import os

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P, srt as SRT
from tests import colour_scenes as SC, ref_colour as R

pytestmark = pytest.mark.gpu


def _gpu(sc, flags=0, with_depths=True, **kw):
    return P.ColourVertices(sc["points"], sc["normals"], sc["cameras"], sc["imgs"], sc["depths"] if with_depths else None, sc["scales"], sc["Rs"],
                            sc["ts"], P.colour_params(flags=flags), with_counts=True, **kw)


def _same(got, ref):
    col, cnt = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in got)
    assert col.dtype == np.uint8 and cnt.dtype == np.int32 and col.shape == ref["colours"].shape
    diff = np.flatnonzero((col != ref["colours"]).any(axis=1) | (cnt != ref["n_views"]))
    assert diff.size == 0, (diff[:10], col[diff[:10]], ref["colours"][diff[:10]], cnt[diff[:10]], ref["n_views"][diff[:10]])


@pytest.mark.parametrize("mapping", ["1", "16"])
@pytest.mark.parametrize("flags", [0, R.BEST])
@pytest.mark.parametrize("name", SC.NAMES)
def test_every_scene_equals_the_restatement(name, flags, mapping, monkeypatch):
    """MVS_COLOUR_MAPPING fixes the mapping: a thread per vertex, and a row of 16 lanes per vertex (N = 1, 16 and 17 views: one lane
    alone, a full row, one more)"""
    monkeypatch.setenv("MVS_COLOUR_MAPPING", mapping)
    _same(_gpu(SC.scene(name), flags), SC.reference(name, flags))


@pytest.mark.parametrize("name", ["O", "Q"])
def test_without_rasters(name):
    """depths = NULL skips C4: the back sheet takes the colours of the front cameras.  The mapping is the call's own choice here"""
    for flags in (0, R.BEST):
        _same(_gpu(SC.scene(name), flags, with_depths=False), SC.reference(name, flags, False))


def test_fill_counts_and_an_empty_call():
    sc = SC.scene("E")
    col = P.ColourVertices(sc["points"], sc["normals"], sc["cameras"], sc["imgs"], params=P.colour_params(fill=(7, 8, 9)))
    ref = SC.reference("E")
    none = ref["n_views"] == 0
    assert none.sum() >= 4 and (col[none] == [7, 8, 9]).all() and np.array_equal(col[~none], ref["colours"][~none])
    got = P.ColourVertices(np.zeros((0, 3)), np.zeros((0, 3)), sc["cameras"], sc["imgs"], with_counts=True)
    assert got[0].shape == (0, 3) and got[1].shape == (0,)


def test_the_device_form_on_a_stream_equals_the_host_form_and_two_runs_agree():
    import torch
    sc = SC.scene("Q")
    for flags in (0, R.BEST):
        host = _gpu(sc, flags)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            dev_in = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("points", "normals", "imgs", "depths")}
        assert torch.cuda.current_stream() != st                    # the inputs are pending on st; the call must order itself there
        run = lambda: P.ColourVertices(dev_in["points"], dev_in["normals"], sc["cameras"], dev_in["imgs"], dev_in["depths"], sc["scales"], sc["Rs"],
                                       sc["ts"], P.colour_params(flags=flags), stream=st.cuda_stream, with_counts=True)
        a, b = run(), run()
        assert all(t.is_cuda for t in a)
        for x, y, z in zip(host, a, b):
            assert x.tobytes() == y.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()
        _same(a, SC.reference("Q", flags))
        bare = P.ColourVertices(dev_in["points"], dev_in["normals"], sc["cameras"], dev_in["imgs"], None, sc["scales"], sc["Rs"], sc["ts"],
                                P.colour_params(flags=flags), stream=st.cuda_stream)
        assert np.array_equal(bare.cpu().numpy(), SC.reference("Q", flags, False)["colours"])


def test_scene_o_on_rasters_the_gpu_rendered():
    """mvs_render_depth_views is bit-equal to tests/ref_render.py on the render tests; here too, so the colours are the same bytes"""
    for name in ("O", "Q"):
        sc = SC.scene(name)
        ras = P.RenderViews(sc["points"], sc["faces"], sc["cameras"], sc["scales"], sc["Rs"], sc["ts"])
        differ = np.argwhere(ras.view(np.uint32) != sc["depths"].view(np.uint32))
        assert len(differ) == 0, f"scene {name}: {len(differ)} pixels differ from the restatement, the first (view, v, u): {differ[:10].tolist()}"
        got = P.ColourVertices(sc["points"], sc["normals"], sc["cameras"], sc["imgs"], ras, sc["scales"], sc["Rs"], sc["ts"], with_counts=True)
        _same(got, SC.reference(name))


def test_the_file_form(tmp_path):
    """scene Q as files — an OBJ with facets, SRT.txt and JPEG frames written by Pillow: ColourModelFiles gives the colours of
    ColourVertices on what the files hold (the geometry and the chain through float32, LoadImages' pixels, the rendered rasters).  The
    same OBJ without `vn` lines takes computed normals; the same without facets has no rasters"""
    from PIL import Image
    sc = SC.scene("Q")
    model, srt, out = str(tmp_path / "deform.obj"), str(tmp_path / "SRT.txt"), str(tmp_path / "coloured.obj")
    IO.WriteObj(model, sc["points"], sc["normals"], sc["faces"])
    IO.write_srt_txt(srt, sc["scales"], sc["Rs"], sc["ts"])
    dirs, at = [], 0
    for k, seq in enumerate(sc["cameras"]):
        d = tmp_path / f"seq{k}"
        d.mkdir()
        dirs.append(str(d) + os.sep)
        for i in range(len(seq)):
            Image.fromarray(sc["imgs"][at + i]).save(str(d / f"{i:05d}.jpg"), "JPEG", quality=95)
        at += len(seq)
    pts, nrm, fac = IO.ReadObj(model)
    s, Rs, ts = IO.read_srt_txt(srt, 2)
    imgs = np.concatenate(P.LoadImages(dirs, sc["cameras"], "RGB"))
    ras = P.RenderViews(pts, fac, sc["cameras"], s, Rs, ts)
    cases = [("with normals", model, nrm, fac, ras)]
    bare = str(tmp_path / "bare.obj")
    IO.WriteObj(bare, sc["points"], None, sc["faces"])
    cases.append(("computed normals", bare, SRT.mesh_vertex_normals(pts, fac), fac, ras))
    cloud = str(tmp_path / "PSR0.obj")
    IO.WriteObj(cloud, sc["points"], sc["normals"], None)
    cases.append(("no facets", cloud, nrm, np.zeros((0, 3), np.int32), None))
    for what, path, normals, faces, depths in cases:
        n = P.ColourModelFiles(path, srt, dirs, sc["cameras"], out)
        want, cnt = P.ColourVertices(pts, normals, sc["cameras"], imgs, depths, s, Rs, ts, with_counts=True)
        assert n == int((cnt > 0).sum()) and n > 300, what
        assert np.array_equal(IO.ReadObjColours(out, "RGB"), want), what
        got = IO.ReadObj(out)
        assert np.array_equal(got[0], pts) and np.array_equal(got[2], faces) and len(got[1]) == len(pts), what
    assert not os.path.exists(str(tmp_path / "seq0" / "DATA"))                                      # nothing but out_obj is written
