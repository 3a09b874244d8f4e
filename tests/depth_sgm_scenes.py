"""The scenes of the mvs_recover_depth_maps_aggregated tests: the rigs, surfaces and textures of tests/depth_refine_scenes.py and
tests/depth_recover_scenes.py, swept over [0.125, 0.375] with that file's parameters.  ``reference(name, variant, flags)`` runs the numpy
restatement (tests/ref_depth_sgm.py) on the cost tables of tests/ref_depth_recover.py once and keeps the result for every test; nobody
changes it.

  A33, B33  as in depth_recover_scenes (B33: depth edges, Xc.z <= 0, levels that leave the reference images)
  A2        L = 2: no level has two neighbours
  A64, A65  A at L = 64 and 65: a lane's chunk of the path kernels exactly full, and one level spilling into the next chunk
  A160, A320  3 and 5 levels per lane: the path kernels hold 4 and 8 (1, 2, 4, 8 and 16 are built; 33, 65, 160, 320 and 1024 run them all)
  A1024     16 levels per lane
  AC        two raster sizes in one call (min_refs 1)
  STRIP     4 frames of 7 x 12 with N = 3: a rectangle 1 pixel wide, every horizontal and diagonal path is one pixel long
  W15       N = 15: a rectangle of 10 x 6
  A33n      A33's images plus seeded noise (NOISE_AMP): the quality scene, restatement only

Every scene runs with the variants ``p4`` and ``p8`` (paths 4 and 8 at the default penalties); A33 also with ``zero`` (p1 = p2 = 0: the
winner-takes-all of the quantised capped cost), ``equal`` (p1 = p2) and ``cap1`` (cost_cap = 1: nearly every S ties, the lowest level
wins)."""
import functools

import numpy as np

from tests import depth_recover_scenes as SC, depth_refine_scenes as RS, ref_depth_recover as R, ref_depth_sgm as A

MARGIN, RANGE_MARGIN = SC.MARGIN, SC.RANGE_MARGIN
STRIP = (4, 7, 12, 4.0, "plane", 13)      # frames, w, h, degrees between frames, surface, seed
NOISE_AMP, NOISE_SEED = 4, 77

# name -> (bases, fields that differ from the scene defaults of depth_recover_scenes)
SCENES = {
    "A33": (("A",), dict(levels=33)),
    "B33": (("B",), dict(levels=33)),
    "A2": (("A",), dict(levels=2)),
    "A64": (("A",), dict(levels=64)),
    "A65": (("A",), dict(levels=65)),
    "A160": (("A",), dict(levels=160)),
    "A320": (("A",), dict(levels=320)),
    "A1024": (("A",), dict(levels=1024)),
    "AC": (("A", "C"), dict(levels=33, min_refs=1)),
    "STRIP": (("STRIP",), dict(levels=33, ssd_win=3)),
    "W15": (("W15",), dict(levels=33, ssd_win=15)),
}
NAMES = tuple(SCENES)
VARIANTS = {"p4": dict(paths=4), "p8": dict(paths=8), "zero": dict(p1=0, p2=0), "equal": dict(p1=256, p2=256), "cap1": dict(cost_cap=1)}
CASES = tuple((n, v) for n in NAMES for v in ("p4", "p8")) + tuple(("A33", v) for v in ("zero", "equal", "cap1"))

# Measured on the restatements alone (python -m tests.depth_sgm_scenes, numpy 1.x, flags = SUBSTEP): accepted pixels, and of them those
# within / beyond one level step of the true disparity, for the plain sweep (ref_depth_recover) and the aggregated one (ref_depth_sgm,
# paths 8, the default penalties) on the same images.  A33n is A33 plus uniform integer noise in [-NOISE_AMP, NOISE_AMP] per byte (seed
# NOISE_SEED), clipped to [0, 255].
QUALITY = {
    "A33": dict(plain=dict(accepted=3826, within=3817, beyond=9), aggregated=dict(accepted=3825, within=3824, beyond=1)),       # of 4278 candidates
    "A33n": dict(plain=dict(accepted=3780, within=3775, beyond=5), aggregated=dict(accepted=3780, within=3780, beyond=0)),
}
# The amplitude was to be the smallest of 4, 8, 16, 32 at which the plain sweep's accepted-and-beyond count at least doubles against the
# noise-free A33 (9).  NONE DOES: the plain sweep's acceptance (ssd_err 12.3, peak 0.9) rejects what the noise spoils, and the count
# falls.  amplitude -> the plain sweep's (accepted, beyond).  A33n therefore stays at the smallest amplitude, 4, and is an easier scene
# than the one that was asked for: on it aggregation removes the few gross errors there are and loses no accepted pixel, no more.
AMPLITUDES = {0: (3826, 9), 4: (3780, 5), 8: (3620, 4), 16: (2136, 0), 32: (0, 0)}
# Every (p1, p2, cost_cap) tried, paths 8 -> the aggregated (accepted, within, beyond) on A33n and on A33; the plain sweep has (3780,
# 3775, 5) and (3826, 3817, 9).  The starting values 64, 1024, 4095 do WORSE than the plain sweep on both: a window that leaves the
# textured surface costs thousands, and one such pixel outweighs every penalty along its paths.  The penalties hardly matter on this
# scene; the cap does, and 255 is the largest tried at which the aggregated call meets both requirements (within >= plain's, beyond <=
# plain's).  The defaults are therefore p1 8, p2 128, cost_cap 255.  At amplitude 8 they give (3619, 3618, 1) against the plain (3620,
# 3616, 4); at 16 (2135, 2135, 0) against (2136, 2136, 0): one accepted pixel fewer.
PENALTIES = {
    (64, 1024, 4095): ((3772, 3755, 17), (3814, 3795, 19)),
    (32, 512, 4095): ((3775, 3758, 17), (3819, 3800, 19)),
    (16, 256, 4095): ((3777, 3760, 17), (3821, 3802, 19)),
    (8, 128, 4095): ((3780, 3763, 17), (3824, 3805, 19)),
    (8, 64, 4095): ((3780, 3763, 17), (3825, 3805, 20)),
    (4, 32, 4095): ((3780, 3763, 17), (3825, 3805, 20)),
    (2, 16, 4095): ((3780, 3763, 17), (3825, 3805, 20)),
    (16, 256, 1023): ((3777, 3769, 8), (3821, 3812, 9)),
    (8, 128, 511): ((3780, 3776, 4), None),
    (16, 256, 511): ((3780, 3776, 4), None),
    (64, 1024, 255): ((3777, 3777, 0), None),
    (32, 256, 255): ((3778, 3778, 0), None),
    (16, 256, 255): ((3780, 3780, 0), None),
    (16, 128, 255): ((3780, 3780, 0), None),
    (8, 128, 255): ((3780, 3780, 0), (3825, 3824, 1)),
    (4, 64, 255): ((3780, 3780, 0), None),
    (8, 128, 127): ((3709, 3709, 0), None),
}


@functools.lru_cache(maxsize=None)
def _frames(base):
    if base != "STRIP":
        return SC._frames(base)
    n, w, h, deg, surface, seed = STRIP
    cams = RS._rig(n, w, h, deg, behind_last=False)
    views = [RS._view(c, surface, seed) for c in cams]
    truth, imgs = np.stack([v[0] for v in views]), np.stack([v[1] for v in views])
    for a in (imgs, truth):
        a.setflags(write=False)
    return cams, imgs, truth


def params_of(name):
    bases, fields = SCENES["A33" if name == "A33n" else name]
    N = 3 if bases[0] in ("STRIP", "W15") else RS.SEQUENCES[bases[0]][3]
    return R.params(**dict(dict(dsp_min=SC.DSP_MIN, dsp_max=SC.DSP_MAX, ssd_err=SC.SSD_ERR, peak=0.9, ssd_win=N, ref_frm_count=5, min_refs=2,
                                flags=R.SUBSTEP), **fields))


@functools.lru_cache(maxsize=None)
def noisy(amp, seed=NOISE_SEED):
    cams, imgs, tr = _frames("A")
    rng = np.random.default_rng(seed)
    out = np.clip(imgs.astype(np.int64) + rng.integers(-amp, amp + 1, size=imgs.shape), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def scene(name):
    """-> (cameras[k], imgs[k]) per sequence, and the R-parameters"""
    if name == "A33n":
        return [_frames("A")[0]], [noisy(NOISE_AMP)], params_of(name)
    seqs = [_frames(b) for b in SCENES[name][0]]
    return [s[0] for s in seqs], [s[1] for s in seqs], params_of(name)


def aparams_of(variant):
    return A.aparams(**VARIANTS[variant])


@functools.lru_cache(maxsize=None)
def plain(name):
    """the plain sweep's restatement with the substep: the cost tables of every frame"""
    if name in SC.SCENES and SC.params_of(name) == params_of(name):
        return SC.reference(name)
    cameras, imgs, p = scene(name)
    return R.recover(cameras, imgs, p)


@functools.lru_cache(maxsize=None)
def reference(name, variant="p8", flags=R.SUBSTEP):
    _, imgs, p = scene(name)
    return A.aggregate(plain(name), imgs, dict(p, flags=flags), aparams_of(variant))


def c_params(p, **kw):
    return SC.c_params(p, **kw)


def c_aparams(variant, **kw):
    from multiviewstitch_amd import processor as P
    return P.depth_aggregate_params(**dict(VARIANTS[variant], **kw))


def _counts(res, tr, p):
    acc = res["level"] >= 0
    step = (p["dsp_max"] - p["dsp_min"]) / (p["levels"] - 1)
    err = np.abs(res["out"][acc].astype(np.float64) - tr[acc])
    return dict(accepted=int(acc.sum()), within=int((err <= step).sum()), beyond=int((err > step).sum()))


@functools.lru_cache(maxsize=None)
def _plain_of(amp):
    """the plain restatement on A's cameras with noise of amplitude ``amp`` (0: A33's own images)"""
    cams, imgs, _ = _frames("A")
    imgs = noisy(amp) if amp else imgs
    return imgs, R.recover([cams], [imgs], params_of("A33"))


def plain_quality(amp):
    return _counts(_plain_of(amp)[1][0], _frames("A")[2], params_of("A33"))


def aggregated_quality(amp, a):
    imgs, pl = _plain_of(amp)
    (ag,) = A.aggregate(pl, [imgs], params_of("A33"), a)
    return _counts(ag, _frames("A")[2], params_of("A33"))


def quality(amp, a):
    """-> the counts of the plain and of the aggregated restatement on A's cameras at noise amplitude ``amp``"""
    return dict(plain=plain_quality(amp), aggregated=aggregated_quality(amp, a))


@functools.lru_cache(maxsize=None)
def quality_of(name):
    """A33 or A33n at the default penalties, paths 8"""
    return quality(NOISE_AMP if name == "A33n" else 0, A.aparams())


if __name__ == "__main__":
    import sys
    import time
    if "quality" in sys.argv[1:] or len(sys.argv) == 1:
        base = quality(0, A.aparams())
        print("A33", base)
        for amp in (4, 8, 16, 32):
            q = quality(amp, A.aparams())
            print("amplitude", amp, q, "plain beyond doubles:", q["plain"]["beyond"] >= 2 * base["plain"]["beyond"])
        for (p1, p2, cap), want in PENALTIES.items():
            got = [aggregated_quality(amp, A.aparams(p1=p1, p2=p2, cost_cap=cap)) for amp in (NOISE_AMP, 0)]
            print("p1 p2 cost_cap", (p1, p2, cap), "A33n", got[0], "A33", got[1], "recorded", want)
    if "margins" in sys.argv[1:] or len(sys.argv) == 1:
        for nm, var in CASES:
            t0 = time.perf_counter()
            for r in reference(nm, var):
                print(nm, var, {k: f"{v:.2e}" for k, v in r["margins"].items()}, "accepted", int((r["level"] >= 0).sum()),
                      "Lmax", max((fr["Lmax"] for fr in r["frames"]), default=0), f"{time.perf_counter() - t0:.1f} s")
