"""Processor::Render on the GPU (R/Processor/Processor.cpp:1140-1192, R/Model2Depth/Model2Depth.cpp:58-190): the batched render of
every camera of every sequence against the oracle's one-camera render of the oracle's inverse map, the mixed-size rule against the
numpy restatement (tests/ref_render.py), the device form, chunking, edge cases, and the files of mvs_processor_render.  Rasters
and files are bit / byte identical."""
import functools

import numpy as np
import pytest

from multiviewstitch_amd import _lib
from multiviewstitch_amd import io as mio
from multiviewstitch_amd import scene as S
from oracle import binding as O
from tests import ref_render as RR
from tests import render_meshes as RM
from tests.util import body_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def proc():
    from multiviewstitch_amd import processor
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return processor


@functools.lru_cache(maxsize=1)
def template():
    sc = S.make_scene(1)                                       # closed template mesh, 3612 vertices
    return sc.verts.copy(), sc.faces.astype(np.int32)


def oracle_views(pts, faces, scales, Rs, ts, cams):
    out = []
    for k, seq in enumerate(cams):
        q = pts if scales is None else O.srt_apply(pts, None, scales[k], Rs[k], ts[k], inverse=True)[0]
        out += [O.render_depth(q, faces, c) for c in seq]
    return out


def test_views_equal_the_oracle(proc):
    pts, faces = template()
    scales, Rs, ts, cams = S.make_stitch_sequences([3, 5, 8, 4], [(96, 72)] * 4, [1.4] * 4, seed=7)
    got = proc.RenderViews(pts, faces, cams, scales, Rs, ts)
    want = oracle_views(pts, faces, scales, Rs, ts, cams)
    assert got.shape == (20, 72, 96)
    for v, w in enumerate(want):
        assert np.array_equal(got[v], w), v
    assert (got > 0).mean() > 0.05 and min((w > 0).mean() for w in want) > 0.01


def test_mixed_sizes_use_the_first_cameras_viewport(proc):
    pts, faces = template()
    sizes = [(80, 60), (64, 48), (100, 70)]
    scales, Rs, ts, cams = S.make_stitch_sequences([2, 3, 2], sizes, [1.4] * 3, seed=9)
    got = proc.RenderViews(pts, faces, cams, scales, Rs, ts)
    assert got.shape == (7, 60, 80)
    v = 0
    for k, seq in enumerate(cams):
        q = O.srt_apply(pts, None, scales[k], Rs[k], ts[k], inverse=True)[0]
        for c in seq:
            want = RR.render(q, faces, c, 80, 60)
            assert np.array_equal(got[v], want), v
            assert (want > 0).mean() > 0.01
            if (c.w, c.h) == (80, 60):
                assert np.array_equal(want, O.render_depth(q, faces, c))
            v += 1


def test_device_form_and_chunks_give_the_same_bytes(proc, monkeypatch):
    import torch
    pts, faces = template()
    scales, Rs, ts, cams = S.make_stitch_sequences([3, 4, 2], [(100, 75)] * 3, [1.4] * 3, seed=3)
    host = proc.RenderViews(pts, faces, cams, scales, Rs, ts)
    dev = torch.device("cuda", 0)
    tp, tf = torch.from_numpy(pts).to(dev), torch.from_numpy(faces).to(dev)
    out = torch.full((9, 75, 100), -1.0, dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        proc.RenderViews((tp.data_ptr(), len(pts)), (tf.data_ptr(), len(faces)), cams, scales, Rs, ts, out_dev=out.data_ptr(),
                         stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), host.view(np.uint32))
    for chunk in ("1", "4"):                                   # fewer views per chunk than views
        monkeypatch.setenv("MVS_RENDER_CHUNK_VIEWS", chunk)
        assert proc.RenderViews(pts, faces, cams, scales, Rs, ts).tobytes() == host.tobytes(), chunk
    assert (host > 0).mean() > 0.05


def test_edge_cases(proc):
    cam, big, tiny = RM.edge_case_cameras()
    pts, faces = RM.edge_case_mesh()                  # eye-plane crossing, screen-covering, zero-area, NaN vertex, a plain triangle
    for c in (cam, big, tiny):
        views = [[c, c], [], [c]]                                                    # an empty middle sequence
        got = proc.RenderViews(pts, faces, views)
        want = O.render_depth(pts, faces, c)
        assert got.shape == (3, c.h, c.w) and all(np.array_equal(g, want) for g in got)
        assert (want > 0).all() and len(np.unique(want)) > 2                          # the big triangle behind, the small one in front
        for f in faces:                                                               # each triangle on its own
            assert np.array_equal(proc.RenderViews(pts, f[None], [[c]])[0], O.render_depth(pts, f[None], c))
        empty = proc.RenderViews(pts, np.zeros((0, 3), np.int32), views)
        assert empty.shape == (3, c.h, c.w) and not empty.any()


def write_inputs(tmp_path, pts, nrm, faces, scales, Rs, ts):
    res = tmp_path / "Result"
    res.mkdir()
    mio.WriteObj(str(res / "deform.obj"), pts, nrm, faces)
    mio.write_srt_txt(str(res / "SRT.txt"), scales, Rs, ts)
    return res


def check_files(res, seq_dirs, cams):
    """every render%d.obj and _depth%d.raw against the oracle on what the entry read (float32 text)"""
    n = len(cams)
    p, nrm, f = mio.ReadObj(str(res / "deform.obj"))
    if len(nrm) == 0:
        nrm = O.vertex_normals(p, f, kind="plyobj")
    s, R, t = mio.read_srt_txt(str(res / "SRT.txt"), n)
    got = {k: (res / f"render{k}.obj").read_bytes() for k in range(n)}
    covered = []
    for k in range(n):
        q, qn = O.srt_apply(p, nrm, s[k], R[k], t[k], inverse=True)
        mio.WriteObj(str(res / f"render{k}.obj"), q, qn, f)                         # (same path: WriteObj prints it in its header)
        assert got[k] == (res / f"render{k}.obj").read_bytes(), k
        for i, c in enumerate(cams[k]):
            want = O.render_depth(q, f, c)
            raw = (seq_dirs[k] / "DATA" / "Render" / f"_depth{i}.raw").read_bytes()
            assert raw == want.astype(np.float32).tobytes(), (k, i)
            covered.append((want > 0).mean())
        if not cams[k]:
            assert not (seq_dirs[k] / "DATA").exists()
    assert min(covered) > 0.01


@pytest.mark.parametrize("with_vn", [True, False])
def test_processor_render_files(proc, tmp_path, with_vn):
    pts, faces = template()
    scales, Rs, ts, cams = S.make_stitch_sequences([2, 3, 1], [(80, 60)] * 3, [1.4] * 3, seed=4)
    cams[2] = []                                                                    # a sequence without cameras
    res = write_inputs(tmp_path, pts, O.vertex_normals(pts, faces, kind="plyobj") if with_vn else None, faces, scales, Rs, ts)
    seq_dirs = [tmp_path / f"seq{k}" for k in range(3)]
    names = [str(seq_dirs[0]) + "/", str(seq_dirs[1]), str(seq_dirs[2])]           # with and without the trailing '/'
    assert proc.Render(str(res / "deform.obj"), str(res / "SRT.txt"), cams, str(res), names) == 5
    check_files(res, seq_dirs, cams)


def test_processor_render_missing_srt_writes_nothing(proc, tmp_path):
    pts, faces = template()
    scales, Rs, ts, cams = S.make_stitch_sequences([2, 1], [(80, 60)] * 2, [1.4] * 2)
    res = write_inputs(tmp_path, pts, None, faces, scales, Rs, ts)
    (res / "SRT.txt").unlink()
    with pytest.raises(_lib.MvsError):
        proc.Render(str(res / "deform.obj"), str(res / "SRT.txt"), cams, str(res), [str(tmp_path / "a"), str(tmp_path / "b")])
    assert sorted(x.name for x in tmp_path.iterdir()) == ["Result"] and [x.name for x in res.iterdir()] == ["deform.obj"]


def test_main_a0_chain(proc, tmp_path):
    """`main -a 0` on files: Processor::Deform writes deform.obj, Processor::Render maps and renders it."""
    from tests.test_io import write_parts
    sc = body_scene()
    res = tmp_path / "Result"
    res.mkdir()
    model, templ, parts, out = (str(res / n) for n in ("Model.obj", "meanbody.obj", "parts", "deform.obj"))
    mio.WriteObj(model, sc["tgt"], sc["t_nrm"], sc["t_faces"])
    mio.WriteObj(templ, sc["src"], sc["s_nrm"], sc["s_faces"])
    write_parts(parts, sc["s_labels"])
    cam_R = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))[0]
    cam_R[2] = sc["view_ray"] / np.linalg.norm(sc["view_ray"])
    st = proc.Deform(model, templ, parts, cam_R, 0.81, out)
    assert st["outer_done"] == 1
    scales, Rs, ts, cams = S.make_stitch_sequences([3, 2], [(80, 60)] * 2, [1.0] * 2, seed=2, dist=6.0)
    mio.write_srt_txt(str(res / "SRT.txt"), scales, Rs, ts)
    seq_dirs = [tmp_path / "s0", tmp_path / "s1"]
    assert proc.Render(out, str(res / "SRT.txt"), cams, str(res), [str(d) for d in seq_dirs]) == 5
    check_files(res, seq_dirs, cams)
