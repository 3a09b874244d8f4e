"""Mesh -> inverse-depth raster (SURVEY §8(f) row 3, R/Model2Depth/Model2Depth.cpp:58-156): known answers for the oracle
(a triangulated depth map rendered back through its own camera), bit-exact parity of the HIP kernels on the GPU."""
import numpy as np
import pytest

from multiviewstitch_amd import scene as S
from tests import ref_render as RR
from tests import render_meshes as RM
from tests.util import scene_and_target


def view_mesh(oracle, config=1, k=0):
    sc, _, _, _ = scene_and_target(config)
    pts, nrm, tex, faces = oracle.depth_to_model(sc.depth[k], sc.cams[k], S.MIN_DSP, S.MAX_DSP, S.SMOOTH)
    return sc, pts, faces, tex


def test_oracle_render_back_reproduces_the_depth_map(oracle):
    """The triangulated raster rendered through its own camera: a pixel centre (i+.5, j+.5) lies on the diagonal
    (j,i)-(j+1,i+1) of the quad Depth2Model splits (Depth2Model.cpp:45-77), and inverse depth is affine in window
    space, so the rendered value is the mean of the two diagonal samples."""
    sc, pts, faces, tex = view_mesh(oracle)
    cam, d = sc.cams[0], sc.depth[0].astype(np.float64)
    r = oracle.render_depth(pts, faces, cam).astype(np.float64)
    valid = (d >= S.MIN_DSP) & (d <= S.MAX_DSP)
    # quads that Depth2Model triangulated completely (both triangles passed its smoothness test)
    quad_of_face = tex[faces].min(1)                                              # raster index of the quad's top-left pixel
    full = (np.bincount(quad_of_face, minlength=d.size) == 2).reshape(d.shape)[:-1, :-1]
    want = 0.5 * (d[:-1, :-1] + d[1:, 1:])
    got = r[:-1, :-1]
    assert full.sum() > 10000 and (got[full] > 0).mean() > 0.999
    hit = full & (got > 0)
    assert np.abs(got[hit] / want[hit] - 1).max() < 2e-4                          # float32 vertex stage + float32 depth buffer
    assert not r[~np.pad(valid[:-1, :-1] | valid[1:, 1:] | valid[1:, :-1] | valid[:-1, 1:], ((0, 1), (0, 1)))].any()   # background stays 0


def test_oracle_render_occlusion_and_clipping(oracle):
    cam = S.Camera(120.0, 120.0, 49.5, 39.5, np.eye(3), np.zeros(3), 100, 80)
    quad = lambda z, s: np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], float)
    pts = np.concatenate([quad(4.0, 1.0), quad(2.0, 0.3), quad(-1.0, 5.0)])       # far wall, near plate, a plate behind the eye
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [8, 9, 10], [8, 10, 11]], np.int32)   # second plate clockwise
    r = oracle.render_depth(pts, faces, cam)
    assert abs(r[40, 50] - 0.5) < 1e-4 and abs(r[40, 30] - 0.25) < 1e-4 and r[2, 2] == 0     # nearest wins, either winding, behind = dropped
    assert set(np.round(np.unique(r), 3)) == {0.0, 0.25, 0.5}


def test_tie_meshes_put_pixel_centres_on_edges_and_depths_in_ties(oracle):
    """What the GPU test below relies on: in these meshes pixel centres have an edge function exactly 0.0, on top or left edges
    (drawn) and on edges of the other kind (not drawn), and pixels get the identical depth from two triangles; the restatement that
    counts them equals the oracle bit for bit."""
    cam = RM.tie_camera()
    _, p, _, _ = RR.glcam(cam)
    assert p["p00"] == 2 and p["p11"] == 2 and p["p02"] == 0 and p["p12"] == 0       # the exact frustum the layout relies on
    seen = {}
    for name, (pts, faces) in RM.tie_meshes().items():
        win = RR.project(pts, cam, cam.w, cam.h)
        assert np.array_equal(win[:, :2], np.round(win[:, :2] * 2) / 2)              # window coordinates are whole or half pixels, exactly
        st = {}
        got = RR.render(pts, faces, cam, stats=st)
        assert np.array_equal(got.view(np.uint32), oracle.render_depth(pts, faces, cam).view(np.uint32)), name
        seen[name] = st
        print(name, st, int((got > 0).sum()), "pixels drawn")
    assert seen["diagonal"]["on_edge_drawn"] == 9 * 7 and seen["diagonal"]["on_edge_skipped"] == 9 * 7   # one of the two triangles of a quad
    assert seen["vertex"]["on_edge_drawn"] == 8 * 10                                 # 9 x 11 centres less one row and one column of the rim
    assert seen["vertex"]["on_edge_skipped"] > 0 and seen["coplanar"]["ties"] > 0
    assert all(v > 0 for v in seen["all"].values())
    vpts, vfaces = RM.tie_meshes()["vertex"]
    drawn = oracle.render_depth(vpts, vfaces, cam)[::-1] > 0                         # window rows (RenderDepth flips them)
    assert drawn[14:24, 15:23].all() and drawn.sum() == 80 and not drawn[13].any() and not drawn[:, 23].any()   # window y points up
    assert (np.bincount(vfaces.ravel()) == 6).sum() == 7 * 9                         # the inner vertices


@pytest.mark.gpu
def test_gpu_render_edge_case_mesh(oracle):
    """the mesh of test_gpu_render_views.py::test_edge_cases through the one-thread-per-triangle rasteriser"""
    from multiviewstitch_amd import processor
    pts, faces = RM.edge_case_mesh()
    for c in RM.edge_case_cameras():
        want = oracle.render_depth(pts, faces, c)
        assert np.array_equal(processor.RenderDepth(pts, faces, c).view(np.uint32), want.view(np.uint32))
        assert (want > 0).all() and len(np.unique(want)) > 2
        for f in faces:                                                               # each triangle on its own
            assert np.array_equal(processor.RenderDepth(pts, f[None], c).view(np.uint32), oracle.render_depth(pts, f[None], c).view(np.uint32)), f
        empty = processor.RenderDepth(pts, np.zeros((0, 3), np.int32), c)
        assert empty.shape == (c.h, c.w) and not empty.any() and not np.signbit(empty).any()


@pytest.mark.gpu
def test_gpu_render_ties_and_on_edge_centres(oracle):
    import torch
    from multiviewstitch_amd import processor
    cam = RM.tie_camera()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    for name, (pts, faces) in RM.tie_meshes().items():
        want = oracle.render_depth(pts, faces, cam)
        assert np.array_equal(processor.RenderDepth(pts, faces, cam).view(np.uint32), want.view(np.uint32)), name
        with torch.cuda.stream(st):
            tp, tf = torch.from_numpy(pts).to(dev), torch.from_numpy(faces).to(dev)
            out = torch.full((cam.h, cam.w), -1.0, dtype=torch.float32, device=dev)
            processor.RenderDepth((tp.data_ptr(), len(pts)), (tf.data_ptr(), len(faces)), cam, out_dev=out.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), name


@pytest.mark.gpu
def test_gpu_render_is_bit_exact(oracle):
    import torch
    from multiviewstitch_amd import processor
    sc, pts, faces, _ = view_mesh(oracle)
    for cam in (sc.cams[0], sc.cams[1]):                     # its own camera, and a view the mesh was not made from
        assert np.array_equal(processor.RenderDepth(pts, faces, cam), oracle.render_depth(pts, faces, cam))
    # closed template mesh, device-resident path
    dev = torch.device("cuda", 0)
    tp, tf = torch.from_numpy(sc.verts).to(dev), torch.from_numpy(sc.faces.astype(np.int32)).to(dev)
    cam = S.Camera(300.0, 300.0, 159.5, 119.5, *S._look_at(np.array([2.5, 1.0, 0.7])), 320, 240)
    out = torch.empty((240, 320), dtype=torch.float32, device=dev)
    processor.RenderDepth((tp.data_ptr(), len(sc.verts)), (tf.data_ptr(), len(sc.faces)), cam, out_dev=out.data_ptr())
    want = oracle.render_depth(sc.verts, sc.faces, cam)
    assert np.array_equal(out.cpu().numpy(), want) and (want > 0).mean() > 0.1
