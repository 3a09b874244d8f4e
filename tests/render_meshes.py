"""Meshes for the render tests that two files share: the edge-case mesh (eye-plane crossing, screen-covering, zero-area, NaN vertex)
and meshes whose pixel centres sit exactly on triangle edges or receive the same depth twice."""
import numpy as np

from multiviewstitch_amd import scene as S


def edge_case_cameras():
    cam = S.Camera(120.0, 120.0, 49.5, 39.5, np.eye(3), np.zeros(3), 100, 80)
    big = S.Camera(150.0, 150.0, 89.5, 69.5, np.eye(3), np.zeros(3), 180, 140)     # spans 6 x 5 tiles
    tiny = S.Camera(30.0, 30.0, 9.5, 5.5, np.eye(3), np.zeros(3), 20, 12)          # one tile
    return cam, big, tiny


def edge_case_mesh():
    tri = lambda *p: np.array(p, float)
    pts = np.concatenate([
        tri([-1, -1, 3.0], [1, -1, 3.0], [0, 1, -1.0]),                              # 0-2: crosses the eye plane
        tri([-500, -500, 5.0], [500, -500, 5.0], [0, 500, 5.0]),                     # 3-5: covers the whole raster
        tri([0, 0, 2.0], [0.1, 0.1, 2.0], [0.2, 0.2, 2.0]),                          # 6-8: zero area
        tri([np.nan, 0, 2.0], [0.3, 0, 2.0], [0, 0.3, 2.0]),                         # 9-11: a NaN vertex
        tri([-0.2, -0.2, 2.5], [0.3, -0.1, 2.5], [0.0, 0.4, 2.0]),                  # 12-14: a plain triangle in front
        tri([7, 7, 7.0], [8, 8, 8.0]),                                               # 15-16: unused vertices
    ])
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 14, 13]], np.int32)
    return pts, faces


# ---- pixel centres exactly on edges, and ties ----
# A 32 x 32 camera with fx = fy = 32, cx = cy = 16, R = I, t = 0 has a symmetric frustum whose float32 entries are exact (p00 = p11 = 2,
# p02 = p12 = 0), so a point (x, y, z) with z a power of two lands on window (16 + 32 x / z, 16 - 32 y / z) without rounding: meshes
# are laid out in window coordinates and taken back to the camera frame exactly.
TIE_W = 32


def tie_camera():
    return S.Camera(32.0, 32.0, 16.0, 16.0, np.eye(3), np.zeros(3), TIE_W, TIE_W)


def from_window(wx, wy, z):
    wx, wy = np.asarray(wx, np.float64), np.asarray(wy, np.float64)
    return np.stack([(wx - 16.0) * z / 32.0, (16.0 - wy) * z / 32.0, np.full(wx.shape, float(z))], axis=-1)


def split_grid(x0, y0, nx, ny, z, step=1.0):
    """nx x ny quads from window (x0, y0), each split along the diagonal (0,0)-(1,1) the way Depth2Model splits a quad
    (Depth2Model.cpp:54-56,67-69) -> (points, faces)"""
    gy, gx = np.mgrid[0:ny + 1, 0:nx + 1]
    pts = from_window(x0 + step * gx.ravel(), y0 + step * gy.ravel(), z)
    v = lambda y, x: y * (nx + 1) + x
    faces = []
    for y in range(ny):
        for x in range(nx):
            faces += [[v(y, x), v(y + 1, x), v(y + 1, x + 1)], [v(y, x), v(y + 1, x + 1), v(y, x + 1)]]
    return pts, np.array(faces, np.int32)


def join(*meshes):
    pts, faces, at = [], [], 0
    for p, f in meshes:
        pts.append(p)
        faces.append(f + at)
        at += len(p)
    return np.concatenate(pts), np.concatenate(faces).astype(np.int32)


def tie_meshes():
    """name -> (points, faces):
    diagonal  vertices on integer window coordinates: every pixel centre of the grid lies on the diagonal its quad is split along
    vertex    vertices on the pixel centres themselves: an inner centre is a vertex shared by six triangles, a centre on the grid's
              rim lies on an edge no second triangle shares — drawn on the top and left rim, not on the bottom and right rim
    coplanar  two overlapping triangles in one plane: every pixel of the overlap gets its depth twice
    all       the three together with a nearer plate in front of a part of them"""
    diagonal = split_grid(3.0, 4.0, 9, 7, 4.0)
    vertex = split_grid(15.5, 13.5, 8, 10, 4.0)
    coplanar = (from_window([2.0, 14.0, 2.0, 5.0, 15.0, 3.0], [13.0, 20.0, 29.0, 14.0, 22.0, 30.0], 8.0),
                np.array([[0, 1, 2], [3, 5, 4]], np.int32))                          # either winding
    plate = split_grid(10.0, 9.0, 2, 2, 2.0, step=4.0)
    return dict(diagonal=diagonal, vertex=vertex, coplanar=coplanar, all=join(diagonal, vertex, coplanar, plate))
