"""Host side of the batched render of Processor::Render (include/mvs.h mvs_render_depth_views*, include/mvs_io.h
mvs_processor_render): the numpy restatement with a separate viewport (tests/ref_render.py) against the oracle, and the argument
checks, which run before any device is needed."""
import ctypes as C

import numpy as np

from multiviewstitch_amd import _lib
from multiviewstitch_amd import scene as S
from tests import ref_render as RR

E_INVALID, E_BAD_MESH = -1, -2


def occlusion_fixture():
    """tests/test_render.py: far wall, near plate (clockwise), a plate behind the eye"""
    cam = S.Camera(120.0, 120.0, 49.5, 39.5, np.eye(3), np.zeros(3), 100, 80)
    quad = lambda z, s: np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], float)
    pts = np.concatenate([quad(4.0, 1.0), quad(2.0, 0.3), quad(-1.0, 5.0)])
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [8, 9, 10], [8, 10, 11]], np.int32)
    return pts, faces, cam


def test_ref_render_equals_the_oracle(oracle):
    pts, faces, cam = occlusion_fixture()
    r = RR.render(pts, faces, cam)
    assert np.array_equal(r, oracle.render_depth(pts, faces, cam)) and set(np.round(np.unique(r), 3)) == {0.0, 0.25, 0.5}
    sc = S.make_scene(0)                                        # 80 x 60
    pts, _, _, faces = oracle.depth_to_model(sc.depth[0], sc.cams[0], S.MIN_DSP, S.MAX_DSP, S.SMOOTH)
    for cam in sc.cams:                                         # its own camera, and a view the mesh was not made from
        want = oracle.render_depth(pts, faces, cam)
        assert np.array_equal(RR.render(pts, faces, cam), want) and (want > 0).mean() > 0.1


def _views(n_seq=2, cams_per_seq=(2, 1)):
    scales, Rs, ts, cams = S.make_stitch_sequences(list(cams_per_seq), [(80, 60)] * n_seq, [2.4] * n_seq)
    return _lib.seq_tables(scales, Rs, ts, cams)


def test_render_views_rejects_bad_arguments():
    L = _lib.lib()
    n, s, R, t, coff, cams = _views()
    pts, faces = np.zeros((3, 3)), np.array([[0, 1, 2]], np.int32)
    out = np.zeros(3 * 60 * 80, np.float32)
    P = _lib.ptr

    def call(pts=pts, V=3, faces=faces, F=1, n=n, s=s, R=R, t=t, coff=coff, cams=cams, zn=0.01, zf=2000.0, out=out, dev=False):
        if dev:
            return L.mvs_render_depth_views_dev(P(pts), V, P(faces), F, n, P(s), P(R), P(t), P(coff), cams, zn, zf, P(out), None)
        return L.mvs_render_depth_views(P(pts), V, P(faces), F, n, P(s), P(R), P(t), P(coff), cams, zn, zf, P(out))

    zero_cams = np.zeros(n + 1, np.int32)
    first_empty = np.array([0, 0, 3], np.int32)                 # cams[0] would belong to sequence 1
    small = (_lib.CCamera * 3)(*cams[:3])
    small[1].w = 0
    no_cx = (_lib.CCamera * 3)(*cams[:3])
    no_cx[2].cx = 0.0
    for dev in (False, True):
        cases = [dict(n=0), dict(coff=None), dict(coff=np.array([1, 2, 3], np.int32)), dict(coff=np.array([0, 3, 2], np.int32)),
                 dict(coff=zero_cams), dict(coff=first_empty), dict(cams=None), dict(cams=small), dict(cams=no_cx),
                 dict(s=None), dict(R=None), dict(t=None), dict(zn=0.0), dict(zn=-1.0), dict(zf=0.01), dict(zf=float("nan")),
                 dict(pts=None), dict(V=0), dict(faces=None), dict(F=-1), dict(out=None)]
        for kw in cases:
            assert call(dev=dev, **kw) == E_INVALID, (dev, kw)
            assert L.mvs_last_error()
    # no SRT at all is the world frame: not an argument error (it fails later for the facet, or without a device)
    assert call(s=None, R=None, t=None, faces=np.array([[0, 1, 3]], np.int32)) == E_BAD_MESH
    assert call(faces=np.array([[0, 1, -1]], np.int32)) == E_BAD_MESH   # the host path checks every facet index
    assert b"facet" in L.mvs_last_error()


def test_processor_render_rejects_bad_arguments(tmp_path):
    L = _lib.lib()
    n, _, _, _, coff, cams = _views()
    obj, srt, res = (str(tmp_path / x).encode() for x in ("deform.obj", "SRT.txt", "Result"))
    dirs = (C.c_char_p * 2)(str(tmp_path / "a").encode(), str(tmp_path / "b").encode())
    nv = C.c_int64(-7)

    def call(obj=obj, srt=srt, n=n, coff=coff, cams=cams, res=res, dirs=dirs, zn=0.01, zf=2000.0):
        return L.mvs_processor_render(obj, srt, n, _lib.ptr(coff), cams, res, dirs, zn, zf, C.byref(nv))

    half_dirs = (C.c_char_p * 2)(str(tmp_path / "a").encode(), None)
    for kw in [dict(obj=None), dict(srt=None), dict(res=None), dict(dirs=None), dict(dirs=half_dirs), dict(n=0), dict(coff=None),
               dict(coff=np.zeros(n + 1, np.int32)), dict(coff=np.array([0, 0, 3], np.int32)), dict(cams=None),
               dict(zn=0.0), dict(zf=0.001)]:
        assert call(**kw) == E_INVALID, kw
    assert nv.value == -7 and not any(tmp_path.iterdir())      # nothing written
