"""numpy restatement of Image3D::GenNewViews (R/Image3D/Image3D.cpp:109-222) and of the background cull of the key points
(R/Processor/Processor.cpp:567-600), in the reference's order of operations.  numpy never contracts a*b+c, so every value is the
literal IEEE one; sin / cos are math.sin / math.cos, the host libm the library calls.  The paint resolves collisions the way the
reference does, by assigning in ascending i (a plain loop over the colliding pixels), independently of the library's gather."""
import math

import numpy as np

INT_MIN = -2147483648
BOTH_EQUAL, U_EQUAL, V_EQUAL, BILINEAR = 0, 1, 2, 3              # the four interpolation branches of :179-211
SURVIVOR, OUTSIDE, UNMAPPED, INVALID, MASKED, LEAVES = range(6)  # what the cull decides for a key point


def cvt_i32(x):
    """(int)x of a double as the reference's x64 build does it: a finite x with |x| < 2^31 truncates toward zero, anything else
    (NaN, +-inf, out of range) gives INT_MIN, which CheckRange rejects."""
    x = np.asarray(x, np.float64)
    ok = np.isfinite(x) & (np.abs(x) < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), float(INT_MIN)).astype(np.int64)


def check_range(u, v, w, h):
    """CheckRange (R/Common/Utils.h:20-22) on ints"""
    return (u >= 0) & (u < w) & (v >= 0) & (v < h)


def mul33(A, B):
    """a0*b0 + a1*b1 + a2*b2, left to right"""
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def angles(view_count, rot):
    """:131-133: the first view_count entries are used"""
    a = [-rot * i for i in range(view_count // 2, 0, -1)] + [rot * i for i in range(0, view_count // 2 + 1)]
    return a[:view_count]


def homography(cam, axis, angle_deg):
    """RotationMatrix (R/Common/Utils.h:124-138) about row `axis` of R, K_ of :123-125, H = K (R_ K_) of :144; Python floats"""
    R = np.asarray(cam.R, np.float64).reshape(3, 3)
    u = [float(R[axis, 0]), float(R[axis, 1]), float(R[axis, 2])]
    angle = angle_deg / 180 * math.pi
    cosine, sine = math.cos(angle), math.sin(angle)
    R_ = [[cosine + u[0] * u[0] * (1 - cosine), u[0] * u[1] * (1 - cosine) - u[2] * sine, u[1] * sine + u[0] * u[2] * (1 - cosine)],
          [u[2] * sine + u[0] * u[1] * (1 - cosine), cosine + u[1] * u[1] * (1 - cosine), -u[0] * sine + u[1] * u[2] * (1 - cosine)],
          [-u[1] * sine + u[0] * u[2] * (1 - cosine), u[0] * sine + u[1] * u[2] * (1 - cosine), cosine + u[2] * u[2] * (1 - cosine)]]
    fx, fy, cx, cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
    K = [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]
    K_ = [[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]]
    return np.array(mul33(K, mul33(R_, K_)), np.float64)


def gen_view(cam, image, H):
    """one pass of the loop of :136-220 -> (img [h, w, 3] uint8 with unpainted pixels 0, texIndex [h*w] int32, diagnostics)"""
    w_, h_ = int(cam.w), int(cam.h)
    scale = 2.0
    scale_ = 1.0 / scale
    scale2_ = scale_ * scale_
    w, h = int(w_ * scale), int(h_ * scale)
    image = np.asarray(image, np.uint8).reshape(h_, w_, 3)
    i = np.arange(w * h, dtype=np.int64)
    with np.errstate(all="ignore"):
        u = cvt_i32((i % w) - w * scale2_)                                                   # :151-152
        v = cvt_i32((i // w) - h * scale2_)
        wf = (H[2, 0] * u + H[2, 1] * v) + H[2, 2]
        uf = ((H[0, 0] * u + H[0, 1] * v) + H[0, 2]) / wf
        vf = ((H[1, 0] * u + H[1, 1] * v) + H[1, 2]) / wf
    inr = check_range(cvt_i32(uf), cvt_i32(vf), w_, h_)                                      # :156
    minu = minv = 1000000000.0
    maxu = maxv = -1000000000.0
    if inr.any():
        bu, bv = u[inr] + w * scale2_, v[inr] + h * scale2_
        minu, maxu, minv, maxv = float(bu.min()), float(bu.max()), float(bv.min()), float(bv.max())
    centerx, centery = (maxu + minu) * 0.5, (maxv + minv) * 0.5
    offsetx, offsety = centerx - w * scale2_, centery - h * scale2_
    # :170-216
    with np.errstate(all="ignore"):
        u11, v11, u22, v22 = np.floor(uf), np.floor(vf), np.ceil(uf), np.ceil(vf)
        ud = cvt_i32(((i % w) - offsetx) + 0.5)
        vd = cvt_i32(((i // w) - offsety) + 0.5)
    ok = check_range(cvt_i32(u11), cvt_i32(v11), w_, h_) & check_range(cvt_i32(u22), cvt_i32(v22), w_, h_) & check_range(ud, vd, w_, h_)
    src = np.flatnonzero(ok)                                                                 # ascending i
    uf, vf, u11, v11, u22, v22 = (a[src] for a in (uf, vf, u11, v11, u22, v22))
    iu1, iv1, iu2, iv2 = (a.astype(np.int64) for a in (u11, v11, u22, v22))
    ueq, veq = np.abs(u11 - u22) <= 1e-9, np.abs(v11 - v22) <= 1e-9
    branch = np.where(ueq & veq, BOTH_EQUAL, np.where(ueq, U_EQUAL, np.where(veq, V_EQUAL, BILINEAR)))
    rgb11, rgb12, rgb21, rgb22 = (image[a, b].astype(np.float64) for a, b in ((iv1, iu1), (iv2, iu1), (iv1, iu2), (iv2, iu2)))
    col = lambda a: a[:, None]
    with np.errstate(all="ignore"):
        s1 = (vf - v11) / (v22 - v11)
        c_u = rgb11 * col(1 - s1) + rgb12 * col(s1)                                          # :190-194
        s1 = (uf - u11) / (u22 - u11)
        c_v = rgb11 * col(1 - s1) + rgb21 * col(s1)                                          # :197-201
        s1, s2, s3, s4 = (u22 - uf) * (v22 - vf), (uf - u11) * (v22 - vf), (u22 - uf) * (vf - v11), (uf - u11) * (vf - v11)
        c_b = ((rgb11 * col(s1) + rgb21 * col(s2)) + rgb12 * col(s3)) + rgb22 * col(s4)      # :204-210
    val = np.where(col(branch == BOTH_EQUAL), rgb11, np.where(col(branch == U_EQUAL), c_u, np.where(col(branch == V_EQUAL), c_v, c_b)))
    val = np.where(np.isfinite(val), val, 0.0)                                               # (branches not taken may divide by zero)
    assert val.min(initial=0.0) >= 0.0 and val.max(initial=0.0) < 256.0
    rgb = np.trunc(val).astype(np.uint8)                                                     # uchar(double)
    tex = np.where(branch == BOTH_EQUAL, cvt_i32(v11 * w_ + u11), cvt_i32(vf + 0.5) * w_ + cvt_i32(uf + 0.5))      # :181, :213
    dest = vd[src] * w_ + ud[src]
    img = np.zeros((h_ * w_, 3), np.uint8)
    tix = np.full(h_ * w_, -1, np.int64)
    taken = np.full(h_ * w_, -1, np.int64)
    writers = np.bincount(dest, minlength=h_ * w_)
    single = writers[dest] == 1
    img[dest[single]], tix[dest[single]], taken[dest[single]] = rgb[single], tex[single], branch[single]
    for k in np.flatnonzero(~single):                                                        # ascending i: a later i overwrites an earlier one
        img[dest[k]], tix[dest[k]], taken[dest[k]] = rgb[k], tex[k], branch[k]
    wneg = np.zeros(w * h, bool)
    wneg[src] = True
    diag = dict(offsetx=offsetx, offsety=offsety, colliding=int((writers >= 2).sum()), max_writers=int(writers.max(initial=0)),
                branches=[int((taken == b).sum()) for b in range(4)], painted=int((taken >= 0).sum()), in_range=int(inr.sum()),
                wf_nonpositive=int((~(wf > 0)).sum()), wf_nonpositive_painting=int((wneg & ~(wf > 0)).sum()), branch_map=taken.reshape(h_, w_))
    return img.reshape(h_, w_, 3), tix.astype(np.int32), diag


def gen_new_views(cams, imgs, view_count, axis, rot_angle):
    """-> views [n, view_count, h, w, 3] uint8, tex [n, view_count, w*h] int32, diagnostics[n][view_count]"""
    ang = angles(view_count, rot_angle)
    views, tex, diags = [], [], []
    for cam, image in zip(cams, imgs):
        out = [gen_view(cam, image, homography(cam, axis, ang[k])) for k in range(view_count)]
        views.append(np.stack([o[0] for o in out])); tex.append(np.stack([o[1] for o in out])); diags.append([o[2] for o in out])
    return np.stack(views), np.stack(tex), diags


def world_point(cam, dsp, idx):
    """Image3D::GetPoint of pixel idx of a valid raster entry: GetWorldCoordFromImg(u, v, 1.0 / depth) (Image3D.cpp:103,
    R/Camera/Camera.cpp:40-44, 61-67), the arithmetic of mvs_depth_unproject"""
    R, t = np.asarray(cam.R, np.float64).reshape(9), np.asarray(cam.t, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        d = 1.0 / dsp.astype(np.float64)
        x, y, z = (idx % cam.w - cam.cx) * d / cam.fx - t[0], (idx // cam.w - cam.cy) * d / cam.fy - t[1], d - t[2]
        return np.stack([(R[0] * x + R[3] * y) + R[6] * z, (R[1] * x + R[4] * y) + R[7] * z, (R[2] * x + R[5] * y) + R[8] * z], 1)


def project(cam, p):
    """GetImgCoordFromWorld (R/Camera/Camera.cpp:45-48, 68-72): integer rounding, no z test"""
    R, t = np.asarray(cam.R, np.float64).reshape(9), np.asarray(cam.t, np.float64).reshape(3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        cx = ((R[0] * x + R[1] * y) + R[2] * z) + t[0]
        cy = ((R[3] * x + R[4] * y) + R[5] * z) + t[1]
        cz = ((R[6] * x + R[7] * y) + R[8] * z) + t[2]
        return cvt_i32(cam.fx * cx / cz + cam.cx + 0.5), cvt_i32(cam.fy * cy / cz + cam.cy + 0.5)


def keypoint_cull(cams, view_count, keys, descs, tex, depths, min_dsp, max_dsp, masks=None):
    """Processor.cpp:567-600 for the lists keys[i] ([k_i, 4] float32 {x, y, s, o}; list i = frame i // view_count, view i % view_count),
    descs[i] ([k_i, 128] float32) or None.  -> (what[i] int per key: SURVIVOR or the test that removed it, keys_out[i], descs_out[i])"""
    n = len(cams)
    w, h = int(cams[0].w), int(cams[0].h)
    tex = np.asarray(tex).reshape(n, view_count, h * w)
    depths = np.asarray(depths, np.float32).reshape(n, h * w)
    what, keys_out, descs_out = [], [], []
    for i, kl in enumerate(keys):
        f, view = divmod(i, view_count)
        kl = np.asarray(kl, np.float32).reshape(-1, 4)
        res = np.full(len(kl), SURVIVOR, np.int64)
        x, y = cvt_i32(kl[:, 0].astype(np.float64)), cvt_i32(kl[:, 1].astype(np.float64))          # the int parameters of GetTexIndex
        res[~check_range(x, y, w, h)] = OUTSIDE
        a = np.flatnonzero(res == SURVIVOR)
        idx = np.full(len(kl), -1, np.int64)
        idx[a] = tex[f, view, y[a] * w + x[a]]
        res[a[idx[a] == -1]] = UNMAPPED
        a = np.flatnonzero(res == SURVIVOR)
        d = depths[f, idx[a]].astype(np.float64)
        res[a[(d < min_dsp) | (d > max_dsp)]] = INVALID                                              # Image3D.cpp:98-101
        if masks is not None:
            a = np.flatnonzero(res == SURVIVOR)
            res[a[np.asarray(masks).reshape(n, h * w)[f, idx[a]] == 0]] = MASKED
        a = np.flatnonzero(res == SURVIVOR)
        p3d = world_point(cams[f], depths[f, idx[a]], idx[a])
        for g in range(n):
            if g != f:
                u, v = project(cams[g], p3d)
                res[a[~check_range(u, v, w, h)]] = LEAVES
        keep = res == SURVIVOR
        what.append(res)
        keys_out.append(kl[keep])
        descs_out.append(None if descs is None else np.asarray(descs[i], np.float32).reshape(-1, 128)[keep])
    return what, keys_out, descs_out
