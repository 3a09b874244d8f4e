"""The scenes of the vertex-colour tests, built on the CPU: images of 40 x 32, at most 3000 vertices and 17 views.  The rasters come from
tests/ref_render.py (the restatement of mvs_render_depth_views, which the render tests hold bit-equal to the GPU), so no scene needs a
GPU to exist.  A scene is a dict(points, normals, faces, cameras (per sequence), imgs [N, h, w, 3], depths [N, h, w] or None, scales,
Rs, ts (or None: the world frame)).

  P     a tessellated textured plane in front of 3 cameras of one sequence; the texture is random bytes ("P") or a linear ramp of 4
        levels per pixel ("P_RAMP": 3 per column and 1 per row)
  O     two parallel sheets whose normals both face the two front cameras, two cameras behind them and one between them: the back
        sheet is hidden from the front cameras by C4 alone, the cameras behind are turned away by C3, the one between has the front
        sheet behind it and most of the back sheet outside its image (C2)
  Q     scene O's geometry and cameras split over two sequences, the second in a frame of its own (scale 1.3, a rotation of 0.7 rad
        about (1, 2, 3), a translation)
  E     hand-placed vertices in the world frame, no rasters: behind camera 0, exactly on x = w - 1 and on x = 0 of camera 0 (powers
        of two throughout, so the projection is exact), outside by 1 / 64 pixel, a NaN normal, facing away, seen by no view, and one
        on the mirror plane of cameras 1 and 2 and outside camera 0, whose Wq are equal bit for bit: the tie of MVS_COLOUR_BEST
  S<V>_<N>  V random points of the plane seen by N cameras: V = 1, 255, 257 and N = 1, 16, 17, so that a row of 16 view-lanes sees one
        view alone, a full row and one more
"""
import functools

import numpy as np

from multiviewstitch_amd import scene as S
from tests import ref_colour as R, ref_render as RR
from tests.depth_recover_scenes import MARGIN  # noqa: F401  (the bound of test_scene_conditions)

W, H = 40, 32
NAMES = ("P", "O", "Q", "E", "S1_1", "S255_16", "S257_17", "S1_17")


def look_at(pos, target, fx=45.0, up=(0.0, -1.0, 0.0)):
    """a camera at pos looking at target: rows of R = right, down, forward; t = -R pos"""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    f = target - pos
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    Rm = np.stack([r, d, f])
    return S.Camera(fx, fx, W / 2 - 0.5, H / 2 - 0.5, Rm, -Rm @ pos, W, H)


def sheet(nx, ny, z, sx=1.0, sy=0.8):
    xs, ys = np.meshgrid(np.linspace(-sx, sx, nx), np.linspace(-sy, sy, ny))
    pts = np.stack([xs.ravel(), ys.ravel(), np.full(nx * ny, z)], axis=1)
    idx = np.arange(nx * ny).reshape(ny, nx)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int32)
    nrm = np.tile(np.array([0.0, 0.0, -1.0]), (nx * ny, 1))
    return pts, nrm, faces


def random_images(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def ramp_images(n):
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    img = np.stack([3 * xs + ys + 10 * ch for ch in range(3)], axis=2).astype(np.uint8)             # at most 3 * 39 + 31 + 20 = 168
    return np.tile(img[None], (n, 1, 1, 1))


def ramp_value(x, y, ch):
    return 3.0 * x + y + 10.0 * ch


def rasters(points, faces, cameras, scales=None, Rs=None, ts=None):
    out = []
    for k, seq in enumerate(cameras):
        pm = points if scales is None else R.map_seq(scales[k], Rs[k], ts[k], points, points)[0]
        out += [RR.render(pm, faces, c, W, H) for c in seq]
    return np.stack(out)


def _world(points, normals, faces, cams, imgs, with_depths=True):
    return dict(points=points, normals=normals, faces=faces, cameras=[cams], imgs=imgs,
                depths=rasters(points, faces, [cams]) if with_depths else None, scales=None, Rs=None, ts=None)


def _o_parts():
    p0, n0, f0 = sheet(24, 20, 0.0)
    p1, n1, f1 = sheet(24, 20, 0.5)
    pts, nrm, faces = np.concatenate([p0, p1]), np.concatenate([n0, n1]), np.concatenate([f0, f1 + len(p0)]).astype(np.int32)
    cams = [look_at((-0.45, 0.1, -3.0), (0, 0, 0)), look_at((0.5, -0.15, -3.1), (0, 0, 0)),
            look_at((0.3, 0.1, 3.6), (0, 0, 0.5)), look_at((-0.35, -0.1, 3.4), (0, 0, 0.5)), look_at((0.03, 0.02, 0.25), (0.03, 0.02, 1.0))]
    return pts, nrm, faces, cams


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def local_camera(c, s, Rs, t):
    """the camera c of the world as a camera of the frame p = s Rs p' + t: q / s = (Rc Rs) p' + (Rc t + tc) / s"""
    Rc, tc = np.asarray(c.R, np.float64).reshape(3, 3), np.asarray(c.t, np.float64).reshape(3)
    return S.Camera(c.fx, c.fy, c.cx, c.cy, Rc @ Rs, (Rc @ np.asarray(t, np.float64) + tc) / s, c.w, c.h)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in ("P", "P_RAMP"):
        pts, nrm, faces = sheet(30, 24, 0.0)
        cams = [look_at((-0.5, 0.05, -3.0), (0, 0, 0)), look_at((0.02, 0.21, -3.05), (0, 0, 0)), look_at((0.6, -0.1, -2.9), (0, 0, 0))]
        return _world(pts, nrm, faces, cams, random_images(3, 11) if name == "P" else ramp_images(3))
    if name == "O":
        pts, nrm, faces, cams = _o_parts()
        return _world(pts, nrm, faces, cams, random_images(5, 12))
    if name == "Q":
        pts, nrm, faces, cams = _o_parts()
        scales = np.array([1.0, 1.3])
        Rs = np.stack([np.eye(3), rodrigues((1, 2, 3), 0.7)])
        ts = np.array([[0.0, 0.0, 0.0], [0.4, -0.3, 0.2]])
        seqs = [[cams[0], cams[4]], [local_camera(c, scales[1], Rs[1], ts[1]) for c in (cams[1], cams[2], cams[3])]]
        return dict(points=pts, normals=nrm, faces=faces, cameras=seqs, imgs=random_images(5, 13),
                    depths=rasters(pts, faces, seqs, scales, Rs, ts), scales=scales, Rs=Rs, ts=ts)
    if name == "E":
        c0 = S.Camera(32.0, 32.0, W / 2 - 0.5, H / 2 - 0.5, np.eye(3), np.zeros(3), W, H)          # x = 16 X + 19.5 at z = 2
        c1 = look_at((1.5, 1.5, -1.0), (0.0, 1.5, 2.0))
        M = np.diag([-1.0, 1.0, 1.0])
        c2 = S.Camera(c1.fx, c1.fy, c1.cx, c1.cy, M @ c1.R @ M, M @ c1.t, W, H)                      # c1 mirrored about x = 0: signs only
        front = [0.0, 0.0, -1.0]
        rows = [([0.1, 0.2, -1.0], front),                     # 0 behind camera 0
                ([1.21875, 0.25, 2.0], front),                 # 1 x = 39 = w - 1 exactly: x0 clamps, ax = 256
                ([-1.21875, -0.25, 2.0], front),               # 2 x = 0 exactly
                ([-1.21875 - 2.0 ** -10, 0.5, 2.0], front),    # 3 x = -1 / 64: outside by a hair
                ([0.3, 0.1, 2.0], [np.nan, 0.0, -1.0]),        # 4 a NaN normal
                ([-0.3, -0.1, 2.0], [0.0, 0.0, 1.0]),          # 5 facing away
                ([100.0, 50.0, 2.0], front),                   # 6 seen by no view
                ([0.0, 1.5, 2.0], front),                      # 7 on the mirror plane, outside camera 0: the tie
                ([0.4, -0.3, 2.5], [0.1, 0.0, -1.0])]          # 8 an ordinary vertex
        pts = np.array([r[0] for r in rows], np.float64)
        nrm = np.array([r[1] for r in rows], np.float64)
        return _world(pts, nrm, np.zeros((0, 3), np.int32), [c0, c1, c2], random_images(3, 14), with_depths=False)
    if name.startswith("S"):
        V, N = (int(v) for v in name[1:].split("_"))
        rng = np.random.default_rng(100 * V + N)
        pts = np.stack([rng.uniform(-1, 1, V), rng.uniform(-0.8, 0.8, V), rng.uniform(-0.05, 0.05, V)], axis=1)
        nrm = np.stack([rng.uniform(-0.3, 0.3, V), rng.uniform(-0.3, 0.3, V), -np.ones(V)], axis=1)
        cams = [look_at((rng.uniform(-1.5, 1.5), rng.uniform(-1, 1), -3.0 + rng.uniform(-0.3, 0.3)), (0, 0, 0)) for _ in range(N)]
        return _world(pts, nrm, np.zeros((0, 3), np.int32), cams, random_images(N, 15 + N), with_depths=False)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, flags=0, with_depths=True):
    """the restatement on a scene, computed once and shared: leave it unchanged"""
    sc = scene(name)
    return R.colour(sc["points"], sc["normals"], sc["cameras"], sc["imgs"], sc["depths"] if with_depths else None, sc["scales"], sc["Rs"],
                    sc["ts"], R.params(flags=flags))
