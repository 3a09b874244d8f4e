"""numpy restatement of the z-buffer render of Model2Depth (R/Model2Depth/Model2Depth.cpp:58-190, R/Camera/Camera.cpp:6-38) with a
viewport that may differ from the camera's own size, as Model2Depth::Run has it (one window of cameras[0][0]'s size, each camera
with its own frustum).  Same stages and operation order as multiviewstitch_amd/csrc/render_dev.h: float32 vertex stage, fp64 edge
functions over pixel centres with the top-left rule, float32 depth, minimum per pixel, RenderDepth's conversion with the row flip.
numpy never contracts a*b+c, and every float32 constant is explicit, so each value is the literal IEEE one."""
import numpy as np

F32 = np.float32


def glcam(cam, znear=0.01, zfar=2000.0):
    """make_glcam: modelview rows, the glFrustum entries, the clipping planes GetClippingPlane recovers (float32 / fp64)."""
    zn, zf = F32(znear), F32(zfar)
    R = np.asarray(cam.R, np.float64).reshape(3, 3).astype(F32)
    t = np.asarray(cam.t, np.float64).reshape(3).astype(F32)
    sgn = np.array([1, -1, -1], F32)
    mv = np.concatenate([R * sgn[:, None], (t * sgn)[:, None]], axis=1)
    cx, cy, fx, fy = F32(cam.cx), F32(cam.cy), F32(cam.fx), F32(cam.fy)
    left = cx / fx * zn
    top = cy / fy * zn
    right = (F32(cam.w) - cx) / cx * left
    bottom0 = (F32(cam.h) - cy) / cy * top
    left = -left
    bottom = -bottom0
    two = F32(2)
    p = dict(p00=two * zn / (right - left), p11=two * zn / (top - bottom), p02=(right + left) / (right - left),
             p12=(top + bottom) / (top - bottom), p22=-(zf + zn) / (zf - zn), p23=F32(-2) * zf * zn / (zf - zn))
    m22, m32 = float(p["p22"]), float(p["p23"])
    return mv, p, m32 / (m22 - 1.0), m32 / (m22 + 1.0)


def project(pts, cam, vw, vh, znear=0.01, zfar=2000.0):
    """glVertex3f of the points (narrowed to float32) through the camera's modelview and frustum, viewport (0, 0, vw, vh):
    window (x, y, z) and w_clip, float32 [V, 4]."""
    mv, p, _, _ = glcam(cam, znear, zfar)
    q = np.asarray(pts, np.float64).reshape(-1, 3).astype(F32)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        xe = ((mv[0, 0] * x + mv[0, 1] * y) + mv[0, 2] * z) + mv[0, 3]
        ye = ((mv[1, 0] * x + mv[1, 1] * y) + mv[1, 2] * z) + mv[1, 3]
        ze = ((mv[2, 0] * x + mv[2, 1] * y) + mv[2, 2] * z) + mv[2, 3]
        xc, yc, zc, wc = p["p00"] * xe + p["p02"] * ze, p["p11"] * ye + p["p12"] * ze, p["p22"] * ze + p["p23"], -ze
        xn, yn, zn = xc / wc, yc / wc, zc / wc
        one, half = F32(1), F32(0.5)
        return np.stack([(xn + one) * (half * F32(vw)), (yn + one) * (half * F32(vh)), (zn + one) * half, wc], axis=1)


def raster(win, faces, vw, vh, stats=None):
    """The depth buffer [vh, vw] (float32, cleared to 1): every (triangle, pixel) test of k_rd_raster, minimum per pixel.
    ``stats`` (a dict) receives how often the top-left rule and the minimum had to decide: ``on_edge_drawn`` = pixel centres with an
    edge function exactly 0.0 that the triangle draws (a top or left edge), ``on_edge_skipped`` = centres that only the rule keeps
    out (inside or on every edge, an edge function 0.0 on an edge of the other kind), ``ties`` = pixels whose final depth two or
    more triangles gave, bit for bit."""
    zbuf = np.ones(vw * vh, F32)
    if stats is not None:
        stats.update(on_edge_drawn=0, on_edge_skipped=0, ties=0)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) == 0:
        return zbuf.reshape(vh, vw)
    A, B, C = win[faces[:, 0]], win[faces[:, 1]], win[faces[:, 2]]
    with np.errstate(all="ignore"):
        ok = (A[:, 3] > 0) & (B[:, 3] > 0) & (C[:, 3] > 0)
        ax, ay, bx, by, cx, cy = (v.astype(np.float64) for v in (A[:, 0], A[:, 1], B[:, 0], B[:, 1], C[:, 0], C[:, 1]))
        za, zb, zc = A[:, 2].astype(np.float64), B[:, 2].astype(np.float64), C[:, 2].astype(np.float64)
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        ok &= (area != 0) & (area == area)
        neg = area < 0
        bx, cx = np.where(neg, cx, bx), np.where(neg, bx, cx)
        by, cy = np.where(neg, cy, by), np.where(neg, by, cy)
        zb, zc = np.where(neg, zc, zb), np.where(neg, zb, zc)
        area = np.where(neg, -area, area)
        minx, maxx = np.fmin(ax, np.fmin(bx, cx)), np.fmax(ax, np.fmax(bx, cx))
        miny, maxy = np.fmin(ay, np.fmin(by, cy)), np.fmax(ay, np.fmax(by, cy))
        ok &= (maxx >= 0) & (minx <= vw) & (maxy >= 0) & (miny <= vh)
        sel = np.flatnonzero(ok)
        ax, ay, bx, by, cx, cy, za, zb, zc, area = (v[sel] for v in (ax, ay, bx, by, cx, cy, za, zb, zc, area))
        minx, maxx, miny, maxy = minx[sel], maxx[sel], miny[sel], maxy[sel]
        i0 = np.fmax(0.0, np.floor(np.fmax(minx, 0.0) - 0.5)).astype(np.int64)
        i1 = np.fmin(float(vw - 1), np.ceil(np.fmin(maxx, float(vw)) - 0.5)).astype(np.int64)
        j0 = np.fmax(0.0, np.floor(np.fmax(miny, 0.0) - 0.5)).astype(np.int64)
        j1 = np.fmin(float(vh - 1), np.ceil(np.fmin(maxy, float(vh)) - 0.5)).astype(np.int64)
    tl = lambda ex, ey: (ey < 0) | ((ey == 0) & (ex < 0))
    tl0, tl1, tl2 = tl(cx - bx, cy - by), tl(ax - cx, ay - cy), tl(bx - ax, by - ay)
    nx, ny = np.maximum(i1 - i0 + 1, 0), np.maximum(j1 - j0 + 1, 0)
    n = nx * ny
    tri = np.repeat(np.arange(len(n)), n)                              # every (triangle, pixel) pair of the ranges
    k = np.arange(len(tri)) - np.repeat(np.cumsum(n) - n, n)
    i = i0[tri] + k % nx[tri]
    j = j0[tri] + k // nx[tri]
    px, py = i + 0.5, j + 0.5
    g = lambda v: v[tri]
    e0 = (g(cx) - g(bx)) * (py - g(by)) - (g(cy) - g(by)) * (px - g(bx))
    e1 = (g(ax) - g(cx)) * (py - g(cy)) - (g(ay) - g(cy)) * (px - g(cx))
    e2 = (g(bx) - g(ax)) * (py - g(ay)) - (g(by) - g(ay)) * (px - g(ax))
    inside = (((e0 > 0) | ((e0 == 0) & g(tl0))) & ((e1 > 0) | ((e1 == 0) & g(tl1))) & ((e2 > 0) | ((e2 == 0) & g(tl2))))
    with np.errstate(all="ignore"):
        z = (((e0 * g(za) + e1 * g(zb)) + e2 * g(zc)) / g(area)).astype(F32)
    keep = inside & (z > 0) & (z < 1)
    np.minimum.at(zbuf, (j * vw + i)[keep], z[keep])
    if stats is not None:
        zero = (e0 == 0) | (e1 == 0) | (e2 == 0)
        stats["on_edge_drawn"] = int((keep & zero).sum())
        stats["on_edge_skipped"] = int((~inside & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)).sum())
        px = (j * vw + i)[keep]
        stats["ties"] = int((np.bincount(px[z[keep] == zbuf[px]], minlength=vw * vh) >= 2).sum())
    return zbuf.reshape(vh, vw)


def convert(zbuf, zn_d, zf_d):
    """RenderDepth (:119-142): rows flipped, z_b -> 1/z_e, 0 where nothing was drawn; float32 [vh, vw]."""
    z_b = zbuf[::-1]
    drawn = ~((z_b >= 1) | (z_b <= 0))
    z_n = F32(2) * z_b - F32(1)
    with np.errstate(all="ignore"):
        z_e = (2.0 * zn_d * zf_d / (zf_d + zn_d - z_n.astype(np.float64) * (zf_d - zn_d))).astype(F32)
        r = (1.0 / z_e.astype(np.float64)).astype(F32)
    return np.where(drawn & (z_e > 1e-6), r, F32(0)).astype(F32)


def render(pts, faces, cam, vw=None, vh=None, znear=0.01, zfar=2000.0, stats=None):
    """One view: the camera's own frustum into a vw x vh viewport (default: the camera's size).  float32 [vh, vw].
    ``stats``: see raster."""
    vw = cam.w if vw is None else vw
    vh = cam.h if vh is None else vh
    _, _, zn_d, zf_d = glcam(cam, znear, zfar)
    return convert(raster(project(pts, cam, vw, vh, znear, zfar), faces, vw, vh, stats), zn_d, zf_d)
