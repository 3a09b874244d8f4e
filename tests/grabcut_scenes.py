"""The scenes of the mvs_grabcut_masks tests: a coloured ellipse on a graded background with sigma-12 noise and a foreground-coloured
clutter patch outside the rectangle, 3 frames per call, seeded.  ``reference(name)`` runs the restatement (tests/ref_grabcut.py) once
per scene and keeps the result: the tests read it, none changes it.
  s1, s2, s3 : 96 x 72 (half 48 x 36), margins hl 0.25, hr 0.1, vl 0.25, vr 0.1, seeds 1..3
  odd        : 97 x 73: the last row and column are unused by rule 1 and clamp in rule 12
  border     : 96 x 72 with hl = vl = 0: the rectangle touches the image border
The ellipse's radii are 0.42 of the rectangle's sides, the largest that keep it inside the rectangle under the seeded jitter.  Two IoU
floors (tests/test_grabcut_host.py): 0.9 where the segmentation lives, on the half-size mask against the ellipse sampled at half size,
and FULL_IOU_FLOOR on the full-size mask.  Rule 12 marks every full pixel whose footprint touches a foreground half pixel: it grows the
upsampled mask by a ring one full pixel wide.  Around an ellipse of semi-axes a, b that ring holds about (1/a + 1/b) of the ellipse's
area; the smallest ellipse here has a = 24.2, b = 17.7 (0.42 * 0.65 * 96 - 2 and 0.42 * 0.65 * 72 - 2), so a segmentation that is exact at half
size scores 1 / (1 + 1/24.2 + 1/17.7) = 0.91 at full size, and 0.9 is out of reach at 96 x 72.  FULL_IOU_FLOOR = 0.85 leaves the segmentation
itself 6 points, less than the 10 the half-size floor allows."""
import functools

import numpy as np

from tests import ref_grabcut as R

GAMMA, ITERS = 50.0, 3
FG = np.array([200.0, 60.0, 40.0])
SCENES = {
    "s1": dict(w=96, h=72, seed=1, margins=(0.25, 0.1, 0.25, 0.1)),
    "s2": dict(w=96, h=72, seed=2, margins=(0.25, 0.1, 0.25, 0.1)),
    "s3": dict(w=96, h=72, seed=3, margins=(0.25, 0.1, 0.25, 0.1)),
    "odd": dict(w=97, h=73, seed=4, margins=(0.25, 0.1, 0.25, 0.1)),
    "border": dict(w=96, h=72, seed=5, margins=(0.0, 0.1, 0.0, 0.1)),
}
FRAMES = 3
FULL_IOU_FLOOR = 0.85


def make_frame(rng, w, h, margins):
    """-> (img [h, w, 3] uint8, truth [h, w] bool: the ellipse)"""
    hl, hr, vl, vr = margins
    x0, x1, y0, y1 = w * hl, w * (1.0 - hr), h * vl, h * (1.0 - vr)              # the rectangle at full size
    cx = 0.5 * (x0 + x1) + rng.uniform(-3, 3)
    cy = 0.5 * (y0 + y1) + rng.uniform(-2, 2)
    rx, ry = 0.42 * (x1 - x0) + rng.uniform(-2, 2), 0.42 * (y1 - y0) + rng.uniform(-2, 2)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    truth = ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1.0
    img = np.empty((h, w, 3))
    img[..., 0] = 40.0 + 50.0 * x / w
    img[..., 1] = 110.0 + 60.0 * y / h
    img[..., 2] = 170.0 - 40.0 * x / w
    img[truth] = FG
    if hl > 0.0:                                                                 # clutter of the ellipse's colour, left of the rectangle
        img[int(0.4 * h):int(0.6 * h), 2:int(x0) - 4] = FG
    else:                                                                        # ... or right of it
        img[int(0.4 * h):int(0.6 * h), int(x1) + 3:w - 1] = FG
    img += rng.normal(0.0, 12.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), truth


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (imgs [3, h, w, 3] uint8, truth [3, h, w] bool, params dict of mvs_grabcut_params fields)"""
    s = SCENES[name]
    rng = np.random.default_rng(1000 + s["seed"])
    fr = [make_frame(rng, s["w"], s["h"], s["margins"]) for _ in range(FRAMES)]
    hl, hr, vl, vr = s["margins"]
    imgs, truth = np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])
    imgs.setflags(write=False)
    return imgs, truth, dict(hl=hl, hr=hr, vl=vl, vr=vr, gamma=GAMMA, iters=ITERS)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's result per frame (ref_grabcut.grabcut)"""
    imgs, _, p = scene(name)
    return tuple(R.grabcut(im, p["hl"], p["hr"], p["vl"], p["vr"], p["gamma"], p["iters"]) for im in imgs)


def half_truth(truth):
    """the ellipse at half size: the top-left pixel of every 2 x 2 block"""
    h, w = truth.shape
    return truth[:2 * (h // 2):2, :2 * (w // 2):2]


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return float((a & b).sum()) / float(max(1, (a | b).sum()))


def equal_caps(gw=23, gh=19):
    """a stand-alone cut case: all capacities equal, in all 8 directions, between a column of sources and a column of sinks whose
    terminal links no minimum cut can afford.  Every straight vertical cut costs the same, so the minimum cuts are many and rule G1
    decides -> (excess [gh, gw], cap [8, gh, gw]) int32"""
    e = np.zeros((gh, gw), np.int32)
    e[:, 0] = 100
    e[:, gw - 1] = -100
    return e, np.full((8, gh, gw), 3, np.int32)
