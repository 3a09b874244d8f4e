"""Inputs that take csrc/align.hip through every data-dependent branch, the CPU-side witnesses that say which side of each branch
an input takes (worked out on the oracle's public calls alone), and an exact restatement of the PCA for inputs at its edges.

  1. posed(...)            body_scene's pieces in other rigid poses, with the ground patch under either end and the view ray of
                           either sign; witness(case, oracle) -> which side of every branch of RemoveGround / InitAlignment /
                           LocalAlignmentCore the case takes; label_edit(...) -> label arrays with one label of a limb group
                           merged into another (the label-set repair of Alignment.cpp:479-498).
  2. tie_case(...)         two coincident far-end points with different labels, a chosen distance apart in index: the first-index
                           rule of k_range decides a swap (Alignment.cpp:513-517,525-528).
  3. pca_cases()           small, degenerate and badly placed selections; pca_reference(...) -> mean, covariance over n - 1 (exact
                           rational arithmetic on the doubles' integer mantissas) and its eigen-decomposition (mpmath, 60 digits).

tests/test_align_cases.py holds the oracle to ORACLE_WORST_*; tests/test_gpu_align_edges.py holds the device to GPU_FACTOR times
that (the block partials are folded in another order than the oracle's running sums; 79728d5 set the factor for the rotations).
"""
from __future__ import annotations

import ctypes as C
import functools
from fractions import Fraction

import mpmath
import numpy as np

from multiviewstitch_amd import scene as S

DIST = 0.81
ARM_L, ARM_R = (1 << 2 | 1 << 3 | 1 << 4), (1 << 5 | 1 << 6 | 1 << 7)
LEG_L, LEG_R = (1 << 8 | 1 << 9), (1 << 11 | 1 << 12)
GROUPS = {"ARM_L": (ARM_L, 4), "ARM_R": (ARM_R, 7), "LEG_L": (LEG_L, 9), "LEG_R": (LEG_R, 12)}
TPB, NBLK = 256, 512                    # the reduction kernels' block and grid (csrc/align.hip)
TRIP = TPB * NBLK                       # one full grid-stride trip: 131072 points
EPS = 2.0 ** -52
DEGENERATE = -9                         # MVS_E_DEGENERATE, and the oracle's status for the same

# a branch decided by the sign of a dot product or by a strict compare of two projections is only a witness if the device, whose
# sums are folded in another order (differences of ~1e-15), must decide it the same way
DOT_MARGIN = 1e-6                       # |dot| of two unit vectors behind a flip
FAR_MARGIN = 1e-9                       # (extreme - runner-up) / extent of a limb's projections: 7 orders above rounding
SIN_MARGIN = 1e-3                       # sine of the angle of a limb's two axes: clear of the acos / cross degeneracy (Utils.h:145-147)

GPU_FACTOR = 10.0
# What oracle.pca showed against pca_reference over pca_cases() (tests/test_align_cases.py prints the measurement), rounded up:
#   barycentre 1.35e-15 of the largest |coordinate| (`far 1e6`), eigenvalues 1.09e-14 of the largest one (`n131071`: running sums
#   of 131 K terms), orthonormality 2.91e-16 (`n255`), K 5.09e-15 (`n131073 masked`) where |axis - axis*| <= K / (relative gap of
#   its eigenvalue to the others)
ORACLE_WORST_BARY = 1.5e-15
ORACLE_WORST_EVAL = 1.2e-14
ORACLE_WORST_ORTH = 3e-16
ORACLE_WORST_AXIS_K = 6e-15
GAP_MIN = 1e-6                          # an axis is compared with the reference's only if its eigenvalue is this far (relative) from the others


def pca_bounds(factor=1.0):
    return dict(bary=factor * ORACLE_WORST_BARY, eval=factor * ORACLE_WORST_EVAL, orth=factor * ORACLE_WORST_ORTH,
                axis_k=factor * ORACLE_WORST_AXIS_K)


# ------------------------------------------------------------------------------------- 1. posed scenes ----
_TILT = np.array([[1, 0, 0], [0, np.cos(0.9), -np.sin(0.9)], [0, np.sin(0.9), np.cos(0.9)]])
# body-frame rotations applied before body_scene's pose: none, half-turns about the two axes perpendicular to the body axis (z),
# and a half-turn after a further tilt (the PCA sign convention, which looks at world coordinates, falls differently)
POSES = {"default": np.eye(3), "half_x": np.diag([1.0, -1.0, -1.0]), "half_y": np.diag([-1.0, 1.0, -1.0]),
         "tilt_half_x": _TILT @ np.diag([1.0, -1.0, -1.0])}


@functools.lru_cache(maxsize=16)
def posed(pose="default", ground_end=-1, view_sign=1, seed=5, n_tmpl=8, n_scan=12):
    """tests/util.body_scene from the same pieces, with the scan (body and ground patch) in the rigid pose R0 @ POSES[pose] instead
    of R0, the ground patch beyond the -z (ground_end = -1, as body_scene) or the +z end of the body, and view_ray times view_sign.
    posed() is body_scene(5, 8, 12) to the bit.  -> the same dictionary."""
    rng = np.random.default_rng(seed)
    stretch = np.array([0.45, 0.6, 2.0])

    def labels_of(d):
        band = np.clip(((d[:, 2] + 1.0) * 4).astype(int), 0, 7)
        return (band * 2 + (d[:, 0] > 0)).astype(np.int32)

    dt, ft = S.geodesic_sphere(n_tmpl)
    src = dt * stretch
    src = src + 0.02 * np.sin(src @ np.array([[1.3, 0.7, -0.4], [-0.9, 1.1, 0.5], [0.3, -0.6, 1.7]]) + [0.1, 0.5, 0.9])
    s_labels = labels_of(dt)
    s_nrm = S.vertex_normals_plyobj(src, ft)
    ds, fs = S.geodesic_sphere(n_scan)
    body = ds * stretch * (1.0 + 0.03 * np.sin(3 * ds[:, 2:3]))
    body[:, 0] += 0.10 * ds[:, 2] ** 2 + 0.05 * ds[:, 2] * ds[:, 1]
    body[:, 1] += 0.06 * np.sin(2.0 * ds[:, 2]) * (1.0 + ds[:, 0])
    ang = 0.5
    R0 = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    R = R0 if pose == "default" else R0 @ POSES[pose]
    s, t = 1.7, np.array([0.4, -0.2, 0.3])
    g = np.linspace(-1.2, 1.2, 17)
    gx, gy = np.meshgrid(g, g)
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -2.15)], 1) + rng.normal(scale=0.004, size=(gx.size, 3))
    if ground_end > 0:
        ground[:, 2] = -ground[:, 2]
    gf = []
    for i in range(16):
        for j in range(16):
            a = i * 17 + j
            gf += [(a, a + 17, a + 18), (a, a + 18, a + 1)]
    tgt = np.concatenate([body, ground]) @ R.T * s + t
    t_faces = np.concatenate([fs, np.array(gf, np.int32) + len(body)]).astype(np.int32)
    t_nrm = S.vertex_normals_plyobj(tgt, t_faces)
    view_ray = view_sign * (R0 @ np.array([0.0, 1.0, 0.0]))
    return dict(src=src, s_nrm=s_nrm, s_faces=ft, s_labels=s_labels, tgt=tgt, t_nrm=t_nrm, t_faces=t_faces,
                view_ray=view_ray, n_body=len(body), s=s, R=R, t=t)


# the family: (pose, ground end, view sign).  tests/test_align_cases.py asserts that over it (with EDITS) every witness takes
# every value; found by trying poses on the oracle until that held
FAMILY = [("default", -1, 1), ("default", -1, -1), ("default", 1, 1), ("half_x", -1, 1), ("half_y", 1, -1), ("tilt_half_x", -1, -1)]

# label edits of LocalAlignmentCore's label arrays: (group, side whose array is edited, label that goes missing, label it is
# merged into) — the lowest label of the group, a middle one (arms), the end label itself
_MERGES = [("ARM_L", 2, 3), ("ARM_L", 3, 4), ("ARM_L", 4, 3), ("ARM_R", 5, 6), ("ARM_R", 6, 5), ("ARM_R", 7, 6),
           ("LEG_L", 8, 9), ("LEG_L", 9, 8), ("LEG_R", 11, 12), ("LEG_R", 12, 11)]
EDITS = [(g, side, a, b) for side in ("scan", "tmpl") for g, a, b in _MERGES]


def label_edit(s_labels, t_labels, edit):
    """-> (s_labels, t_labels) with edit = (group, side, missing, into) applied (None: unchanged)"""
    if edit is None:
        return s_labels, t_labels
    _, side, missing, into = edit
    sl, tl = s_labels.copy(), t_labels.copy()
    arr = tl if side == "scan" else sl
    arr[arr == missing] = into
    return sl, tl


def _label_set(labels, mask):
    out = 0
    for v in np.unique(labels):
        if 0 <= v < 32 and (mask >> int(v)) & 1:
            out |= 1 << int(v)
    return out


def _popc(x):
    return bin(x).count("1")


def _lowest(x):
    return x & -x


def _far(pts, labels, mask, axis, centre):
    """first index of the largest and of the smallest projection of the points selected by mask on axis, their labels, and the
    margin of each extreme to the runner-up among the points that do not coincide with it, over the extent"""
    idx = np.flatnonzero((np.right_shift(mask, labels.astype(np.int64)) & 1).astype(bool))
    t = (pts[idx] - centre) @ axis / (axis @ axis)
    out = {}
    for name, key in (("hi", t), ("lo", -t)):
        k = int(np.argmax(key))                                   # (first maximum)
        other = np.any(pts[idx] != pts[idx[k]], axis=1)
        margin = (key[k] - key[other].max()) / (t.max() - t.min()) if other.any() else np.inf
        out[name] = dict(index=int(idx[k]), label=int(labels[idx[k]]), margin=float(margin))
    return out


def limb_witness(oracle, src, s_labels, tgt, t_labels, mask, label):
    """which side of every branch of LocalAlignmentCore (csrc/align.hip local_core_dev; Alignment.cpp:423-546) these arrays take,
    from oracle.pca and the label arrays; `status` is the oracle's own (0, or -9 where it finds no extent)."""
    w = dict(status=0)
    try:
        R, t, s = oracle.local_alignment_core(src, s_labels, tgt, t_labels, mask, label)
        w.update(R=R, t=t, scale=s, finite=bool(np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s)))
    except RuntimeError as e:
        if not str(e).endswith(f"-> {DEGENERATE}"):
            raise
        w["status"] = DEGENERATE
        return w
    bs, _, axs, _ = oracle.pca(src, s_labels, mask)
    bt, _, axt, _ = oracle.pca(tgt, t_labels, mask)
    w["flip_dot"] = float(axs[0] @ axt[0])
    w["flip"] = w["flip_dot"] < 0
    a_t = -axt[0] if w["flip"] else axt[0]
    w["sin_axes"] = float(np.linalg.norm(np.cross(axs[0], a_t)))
    sset, tset = _label_set(s_labels, mask), _label_set(t_labels, mask)
    w["sets"] = "<" if _popc(sset) < _popc(tset) else (">" if _popc(sset) > _popc(tset) else "=")
    if w["sets"] == "<":
        tset &= ~_lowest(tset & ~sset)
    elif w["sets"] == ">":
        sset &= ~_lowest(sset & ~tset)
    fs, ft = _far(src, s_labels, sset, axs[0], bs), _far(tgt, t_labels, tset, a_t, bt)
    w["lab1_eq"], w["lab2_eq"] = fs["hi"]["label"] == label, ft["hi"]["label"] == label
    w["far_src"], w["far_tgt"] = fs, ft
    w["margin"] = min(fs["hi"]["margin"], fs["lo"]["margin"], ft["hi"]["margin"], ft["lo"]["margin"])
    return w


def stage_inputs(case, oracle):
    """what the stage-by-stage checks hand to each stage (as tests/test_align.py does): the oracle's trimmed scan, ground ray,
    initial alignment, moved template and scan labels"""
    gr, p, n, f = oracle.remove_ground(case["tgt"], case["t_nrm"], case["t_faces"], DIST)
    R, t, s = oracle.init_alignment(case["src"], p, gr, case["view_ray"])
    moved = s * case["src"] @ R.T + t
    tl = oracle.part_recog(moved, case["s_labels"], p)
    return dict(ground_ray=gr, p=p, n=n, f=f, R=R, t=t, scale=s, moved=moved, t_labels=tl)


@functools.lru_cache(maxsize=16)
def family_witness(key, oracle):
    """witness(posed(*key), oracle), computed once per session (the CPU conditions and the GPU parity read the same one)"""
    return witness(posed(*key), oracle)


def witness(case, oracle, edits=EDITS):
    """-> which (1 / 2: the ground on the negative / positive side of the whole scan's first pivot, align.hip:721), the ground and
    view flips of InitAlignment (:760-761) with the dot products behind them, and per limb group and label edit limb_witness()"""
    _, _, ax, _ = oracle.pca(case["tgt"])
    st = stage_inputs(case, oracle)
    gr = st["ground_ray"]
    assert np.array_equal(gr, -ax[0]) or np.array_equal(gr, ax[0])
    w = dict(which=1 if np.array_equal(gr, -ax[0]) else 2, stage=st)
    _, _, axt, _ = oracle.pca(st["p"])
    w["ground_dot"], w["view_dot"] = float(gr @ axt[0]), float(case["view_ray"] @ axt[2])
    w["ground_flip"], w["view_flip"] = w["ground_dot"] < 0, w["view_dot"] < 0
    w["limbs"] = {}
    for edit in [None] + list(edits):
        sl, tl = label_edit(case["s_labels"], st["t_labels"], edit)
        for name, (mask, label) in GROUPS.items():
            if edit is None or edit[0] == name:
                w["limbs"][(name, edit)] = limb_witness(oracle, st["moved"], sl, st["p"], tl, mask, label)
    return w


# ------------------------------------------------------------------------- 2. ties at the far end of a limb ----
# distance in index between the two coincident points: the next lane of a wave, the next wave of a block, the next block, the same
# thread one grid-stride trip later — and one trip less one block: the LATER index sits in the EARLIER block, so range_fold has to
# compare indices rather than keep the block it met first
TIE_DISTANCES = (1, 64, TPB, TRIP, TRIP - TPB)
TIE_LANE = TPB + 37                     # the earlier of the two sits here modulo TPB * k: lane 37 of wave 0, not in block 0
PAD_LABEL = 14                          # a label of no limb group


def tie_case(pts, labels, mask, label, index, distance, order):
    """pts / labels with an exact copy of point `index` (the far end of the group `mask`), `distance` entries after
    (order = "after") or before ("before") it; the copy carries another label of the group so that exactly one of the two is
    `label`; the room between them is padded with points of PAD_LABEL at the array's centre.
    -> (pts, labels, labels with the two labels exchanged)"""
    lead = (TIE_LANE - index) % TPB
    if index + lead < TPB:
        lead += TPB
    centre = pts.mean(0)
    mine = int(labels[index])
    if mine == label:
        other = next(v for v in range(31, -1, -1) if (mask >> v) & 1 and v != label and (labels == v).any())
    else:
        other = label
    P = lambda k: np.tile(centre, (k, 1))                                        # noqa: E731
    L = lambda k: np.full(k, PAD_LABEL, np.int32)                                # noqa: E731
    pair = (mine, other) if order == "after" else (other, mine)
    out_p = np.concatenate([P(lead), pts[:index], pts[index:index + 1], P(distance - 1), pts[index:index + 1], pts[index + 1:]])
    lab = lambda a, b: np.concatenate([L(lead), labels[:index], [a], L(distance - 1), [b], labels[index + 1:]]).astype(np.int32)   # noqa: E731
    first = lead + index
    assert np.array_equal(out_p[first], out_p[first + distance]) and first % TPB == TIE_LANE % TPB and first >= TPB
    return np.ascontiguousarray(out_p), lab(*pair), lab(*pair[::-1])


TIE_GROUPS = {"tmpl": "ARM_L", "scan": "LEG_R"}


def tie_family(case, oracle):
    """-> list of (name, src, s_labels, tgt, t_labels, mask, label, s_labels', t_labels') over sides x TIE_DISTANCES x orders, the
    primed arrays with the two coincident points' labels exchanged"""
    st = stage_inputs(case, oracle)
    out = []
    for side, gname in TIE_GROUPS.items():
        mask, label = GROUPS[gname]
        w = limb_witness(oracle, st["moved"], case["s_labels"], st["p"], st["t_labels"], mask, label)
        assert w["status"] == 0 and w["sets"] == "="
        for d in TIE_DISTANCES:
            for order in ("after", "before"):
                if side == "tmpl":
                    p, l1, l2 = tie_case(st["moved"], case["s_labels"], mask, label, w["far_src"]["hi"]["index"], d, order)
                    out.append((f"{side} {gname} {d:+d} {order}", p, l1, st["p"], st["t_labels"], mask, label, l2, st["t_labels"]))
                else:
                    p, l1, l2 = tie_case(st["p"], st["t_labels"], mask, label, w["far_tgt"]["hi"]["index"], d, order)
                    out.append((f"{side} {gname} {d:+d} {order}", st["moved"], case["s_labels"], p, l1, mask, label, case["s_labels"], l2))
    return out


def label31_arrays(case, oracle, edit=None):
    """the left arm's LocalAlignmentCore input with its end label 4 renamed 31 (and `edit` applied): group and label with bit 31
    -> (src, s_labels, tgt, t_labels, mask, label)"""
    st = stage_inputs(case, oracle)
    sl, tl = label_edit(case["s_labels"], st["t_labels"], edit)
    sl, tl = np.where(sl == 4, 31, sl).astype(np.int32), np.where(tl == 4, 31, tl).astype(np.int32)
    return st["moved"], sl, st["p"], tl, (1 << 2 | 1 << 3 | 1 << 31), 31


# --------------------------------------------------------------------------------- 3. the PCA at its edges ----
SEED = 20261020


def _cloud(rng, n, spread=(5.0, 2.0, 0.7)):
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return rng.normal(size=(n, 3)) * spread @ q


@functools.lru_cache(maxsize=1)
def pca_cases():
    """name -> (pts, labels or None, mask): random anisotropic clouds of n around the minimum, a wave, a block and one full
    grid-stride trip, bare and behind a label mask; collinear, coplanar, coincident, two-point and far-away clouds; label 31."""
    rng = np.random.default_rng(SEED)
    F = {}
    for n in (2, 3, 4, 63, 64, 65, TPB - 1, TPB, TPB + 1, TRIP - 1, TRIP, TRIP + 1):
        p = _cloud(rng, n)
        F[f"n{n}"] = (p, None, 0)
        lab = rng.choice(np.array([1, 4, 9, 14, 31], np.int32), size=n)
        lab[[0, n - 1]] = (4, 31)                                                 # (the first and the last entry are selected)
        F[f"n{n} masked"] = (p, lab, 1 << 4 | 1 << 31 | 1 << 9)
    t = rng.integers(-50, 51, size=(300, 1)).astype(np.float64)
    F["collinear"] = (np.array([0.5, -1.25, 3.0]) + t * np.array([2.0, -3.0, 1.0]), None, 0)          # (exact in doubles)
    uv = rng.integers(-50, 51, size=(300, 2)).astype(np.float64)
    F["coplanar"] = (np.array([0.5, -1.25, 3.0]) + uv[:, :1] * np.array([2.0, -3.0, 1.0]) + uv[:, 1:] * np.array([1.0, 1.0, 4.0]), None, 0)
    F["coplanar z=0"] = (np.concatenate([_cloud(rng, 300)[:, :2], np.zeros((300, 1))], 1), None, 0)
    F["two points"] = (np.array([[0.3, -1.7, 2.2], [1.1, 0.4, -0.9]]), None, 0)
    F["two points of five"] = (rng.normal(size=(5, 3)), np.array([3, 0, 3, 7, 7], np.int32), 1 << 7)
    F["far 1e6"] = (_cloud(rng, 300, (1.0, 0.5, 0.2)) + 1e6, None, 0)
    F["far 1e6 masked"] = (_cloud(rng, 600, (1.0, 0.5, 0.2)) + 1e6, rng.integers(0, 4, 600).astype(np.int32), 1 << 2)
    lab = rng.integers(28, 32, 500).astype(np.int32)
    F["label 31 only"] = (_cloud(rng, 500), lab, 1 << 31)
    return F


@functools.lru_cache(maxsize=1)
def coincident_cases():
    """name -> (pts, n * EPS bound factor): all points identical.  Dyadic coordinates: every sum is exact in any order, the
    covariance is exactly zero.  Other coordinates: the barycentre of n copies of x is off x by at most n * EPS * |x| in any
    summation order, so every eigenvalue is at most n / (n - 1) * 3 * (n * EPS * max|x|)^2."""
    x = np.array([0.5, -1.25, 3.0])
    y = np.array([0.1, -0.7, 1e3 / 3])
    return {"dyadic 2": (np.tile(x, (2, 1)), True), "dyadic 300": (np.tile(x, (300, 1)), True), "dyadic trip+1": (np.tile(x, (TRIP + 1, 1)), True),
            "decimal 3": (np.tile(y, (3, 1)), False), "decimal 300": (np.tile(y, (300, 1)), False)}


def coincident_eval_bound(p):
    n = len(p)
    return 6.0 * (n * EPS * np.abs(p).max()) ** 2


def degenerate_selections():
    """name -> (pts, n, labels, mask) selecting 0 or 1 points"""
    rng = np.random.default_rng(SEED)
    p = rng.normal(size=(300, 3))
    lab = rng.integers(0, 8, 300).astype(np.int32)
    one = lab.copy()
    one[123] = 20
    return {"mask matches nothing": (p, 300, lab, 1 << 9), "mask == 0 with labels": (p, 300, lab, 0), "mask matches one": (p, 300, one, 1 << 20),
            "n == 0": (p, 0, None, 0), "n == 0 with labels": (p, 0, lab, 0xff), "n == 1": (p, 1, None, 0)}


def _exact_ints(p):
    """doubles (n, 3) -> (object array of Python ints X, E) with p == X * 2**E exactly"""
    m, e = np.frexp(p)
    mant = np.rint(np.ldexp(m, 53)).astype(np.int64)
    ex = e.astype(np.int64) - 53
    E = int(ex[mant != 0].min()) if (mant != 0).any() else 0
    sh = np.where(mant != 0, ex - E, 0)
    X = np.array([int(a) << int(s) for a, s in zip(mant.ravel().tolist(), sh.ravel().tolist())], dtype=object).reshape(p.shape)
    return X, E


def pca_reference(pts, labels=None, mask=0, digits=60):
    """PointSetUtils::SetInput + CalcPivots in exact / 60-digit arithmetic: the mean and the covariance over n - 1 as exact
    rationals of the doubles, the eigen-decomposition by mpmath.  -> dict(n, bary (3 mpf), bbox (2, 3) doubles, evals (3 mpf,
    largest first), axes (3 rows of 3 mpf, sign convention of pca_finish applied), gaps (relative to evals[0]), scale)"""
    p = pts if labels is None else pts[(np.right_shift(np.uint64(mask), labels.astype(np.uint64)) & np.uint64(1)).astype(bool)]
    n = len(p)
    X, E = _exact_ints(p)
    sx = [sum(X[:, c].tolist()) for c in range(3)]
    sxy = [[sum((X[:, a] * X[:, b]).tolist()) for b in range(3)] for a in range(3)]
    with mpmath.workdps(digits):
        two = mpmath.mpf(2)
        q = lambda fr: mpmath.mpf(fr.numerator) / mpmath.mpf(fr.denominator)          # noqa: E731
        bary = [q(Fraction(sx[c], n)) * two ** E for c in range(3)]
        cov = mpmath.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                cov[a, b] = q(Fraction(sxy[a][b] * n - sx[a] * sx[b], n * (n - 1))) * two ** (2 * E)
        ev, Q = mpmath.eigsy(cov)
        order = [2, 1, 0]
        evals = [ev[k] for k in order]
        axes = []
        for k in order:
            a = [Q[r, k] for r in range(3)]
            ln = mpmath.sqrt(sum(v * v for v in a))
            a = [v / ln for v in a]
            mags = [abs(v) for v in a]
            big = a[0] if (mags[0] >= mags[1] and mags[0] >= mags[2]) else (a[1] if mags[1] >= mags[2] else a[2])
            axes.append([-v for v in a] if big < 0 else a)
        top = evals[0]
        gaps = [float(min(abs(evals[i] - evals[j]) for j in range(3) if j != i) / top) if top > 0 else 0.0 for i in range(3)]
    return dict(n=n, bary=bary, bbox=np.stack([p.min(0), p.max(0)]), evals=evals, axes=axes, gaps=gaps, scale=float(np.abs(p).max()))


@functools.lru_cache(maxsize=64)
def pca_reference_of(name):
    return pca_reference(*pca_cases()[name])


def pca_errors(got, ref, digits=60):
    """got = (bary, bbox, axes, evals) of oracle.pca or alignment.pca against pca_reference: only what is unique.
    -> dict(bary: / largest |coordinate|, bbox: exact?, eval: / largest eigenvalue, orth: max |A A^T - I|, sign: the convention
    holds on got's own axes, axis_k: max over the axes with a gap >= GAP_MIN of |axis - axis*| * gap)"""
    b, bb, ax, ev = got
    with mpmath.workdps(digits):
        e_b = float(max(abs(mpmath.mpf(float(b[c])) - ref["bary"][c]) for c in range(3))) / max(ref["scale"], np.finfo(float).tiny)
        top = ref["evals"][0]
        e_v = float(max(abs(mpmath.mpf(float(ev[i])) - ref["evals"][i]) for i in range(3)) / top) if top > 0 else float(np.abs(ev).max())
        k = 0.0
        for i in range(3):
            if ref["gaps"][i] >= GAP_MIN:
                d = float(max(abs(mpmath.mpf(float(ax[i][c])) - ref["axes"][i][c]) for c in range(3)))
                k = max(k, d * ref["gaps"][i])
    sign = all(a[np.argmax(np.abs(a))] > 0 for a in ax)                 # (np.argmax: the first maximum, as pca_finish's >= chain)
    return dict(bary=e_b, bbox=bool(np.array_equal(bb, ref["bbox"])), eval=e_v, orth=float(np.abs(ax @ ax.T - np.eye(3)).max()),
                sign=bool(sign and np.isfinite(ax).all()), axis_k=k)


# the entries by their C signatures, for what the Python wrappers hide: the status, and whether the outputs were written
SENTINEL = 7.25


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_pca(fn, pts, n, labels, mask):
    """fn = oracle.lib().orc_pca or the engine's mvs_pca -> (status, the four output arrays, pre-filled with SENTINEL)"""
    pts = np.ascontiguousarray(pts, np.float64)
    lab = None if labels is None else np.ascontiguousarray(labels, np.int32)
    out = [np.full(k, SENTINEL) for k in (3, 6, 9, 3)]
    rc = fn(_vp(pts), C.c_int64(n), _vp(lab), C.c_uint32(mask), *[_vp(o) for o in out])
    return rc, out


def raw_remove_ground(fn, pts, faces):
    """fn = orc_remove_ground or mvs_remove_ground -> (status, V, F, pts, normals, faces, ground_ray) after the call"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3).copy()
    nr = p[::-1].copy() + 1.0
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).copy()
    V, F, gr = C.c_int64(len(p)), C.c_int64(len(f)), np.full(3, SENTINEL)
    hold = np.zeros(4)                                                   # (an address for empty arrays)
    rc = fn(C.byref(V), _vp(p if len(p) else hold), _vp(nr if len(p) else hold), C.byref(F), _vp(f) if len(f) else None, C.c_double(DIST), _vp(gr))
    return rc, V.value, F.value, p, nr, f, gr
