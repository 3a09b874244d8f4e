"""Shared helpers of the test-suite: scenes -> target point sets through the ORACLE (checker side); checks of engine
statistics and state against an oracle trajectory."""
import functools
import os

import numpy as np

from multiviewstitch_amd import scene as S
from oracle import binding as O


@functools.lru_cache(maxsize=8)
def scene_and_target(config, smooth=S.SMOOTH, **kw):
    sc = S.make_scene(config, **kw)
    tp, tn = [], []
    for k in range(len(sc.cams)):
        pts, nrm, _, _ = O.depth_to_model(sc.depth[k], sc.cams[k], S.MIN_DSP, S.MAX_DSP, smooth)
        s, R, t = sc.srt[k]
        w, n = O.srt_apply(pts, nrm, s, R, t)
        tp.append(w)
        tn.append(n)
    return sc, np.concatenate(tp), np.concatenate(tn), [len(x) for x in tp]


def rms(a, b):
    d = np.asarray(a) - np.asarray(b)
    return float(np.sqrt(np.mean(np.sum(d.reshape(-1, d.shape[-1]) ** 2, axis=1))))


@functools.lru_cache(maxsize=4)
def body_scene(seed=5, n_tmpl=8, n_scan=12):
    """Synthetic stand-in for the template / scan pair of Processor::Deform (R/Processor/Processor.cpp:1119-1131):
    an elongated closed template with 16 part labels (stripes of enum PART), a denser scan = similarity-moved,
    slightly deformed copy with a disconnected ground patch under its far end."""
    rng = np.random.default_rng(seed)
    stretch = np.array([0.45, 0.6, 2.0])

    def labels_of(d):                                  # 16 parts: 8 bands along the axis x 2 sides; limbs come out as bands
        band = np.clip(((d[:, 2] + 1.0) * 4).astype(int), 0, 7)
        return (band * 2 + (d[:, 0] > 0)).astype(np.int32)

    dt, ft = S.geodesic_sphere(n_tmpl)
    src = dt * stretch
    src = src + 0.02 * np.sin(src @ np.array([[1.3, 0.7, -0.4], [-0.9, 1.1, 0.5], [0.3, -0.6, 1.7]]) + [0.1, 0.5, 0.9])   # break the mirror symmetries (no ties)
    s_labels = labels_of(dt)
    s_nrm = S.vertex_normals_plyobj(src, ft)
    ds, fs = S.geodesic_sphere(n_scan)
    body = ds * stretch * (1.0 + 0.03 * np.sin(3 * ds[:, 2:3]))
    body[:, 0] += 0.10 * ds[:, 2] ** 2 + 0.05 * ds[:, 2] * ds[:, 1]      # bend + shear: limb axes differ from the template's
    body[:, 1] += 0.06 * np.sin(2.0 * ds[:, 2]) * (1.0 + ds[:, 0])
    ang = 0.5
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    s, t = 1.7, np.array([0.4, -0.2, 0.3])
    # ground patch: regular grid just beyond the -z end, not connected to the body
    g = np.linspace(-1.2, 1.2, 17)
    gx, gy = np.meshgrid(g, g)
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -2.15)], 1) + rng.normal(scale=0.004, size=(gx.size, 3))
    gf = []
    for i in range(16):
        for j in range(16):
            a = i * 17 + j
            gf += [(a, a + 17, a + 18), (a, a + 18, a + 1)]
    tgt = np.concatenate([body, ground]) @ R.T * s + t
    t_faces = np.concatenate([fs, np.array(gf, np.int32) + len(body)]).astype(np.int32)
    t_nrm = S.vertex_normals_plyobj(tgt, t_faces)
    view_ray = R @ np.array([0.0, 1.0, 0.0])
    return dict(src=src, s_nrm=s_nrm, s_faces=ft, s_labels=s_labels, tgt=tgt, t_nrm=t_nrm, t_faces=t_faces,
                view_ray=view_ray, n_body=len(body), s=s, R=R, t=t)


def counts_match(got, ref, max_result=10000):
    """{ball population, survivors of the normal test} per node.  A ball with >= max_result members drops the node — the
    reference's radiusSearch returns at most max_result neighbours (R/Deformation/Deformation.cpp:286-297) — and the engine
    stops counting there: for such nodes only "full" is compared, for all others both numbers exactly."""
    got, ref = np.asarray(got), np.asarray(ref)
    full = ref[:, 0] >= max_result
    return bool(np.array_equal(got[~full], ref[~full]) and (got[full, 0] >= max_result).all())


def oracle_threads(oracle):
    """the oracle's OpenMP threads for a long run (results are bit-identical on any count); pair with set_threads(1)"""
    oracle.set_threads(min(16, len(os.sched_getaffinity(0))))


def check_pass(st, so, tag, rtol=None):
    """the engine's last pass of a call (``st``) == the oracle's pass (``so`` of Deform.iterate, plus ``ratio``, its stop-rule
    ratios |E(t-1)-E(t)|/E(t)): integers equal, energies to ``rtol`` (None: not compared).  On a mismatch the message shows the ratios (against
    arap_tol) and GPU - oracle energies: a stop decided on a knife-edge reads differently from a wrong result.
    -> the largest relative energy difference."""
    why = (f"{tag}: GPU n_valid {st['n_valid']} arap_iters_run {st['arap_iters_run']}, oracle {so['n_valid']} "
           f"{so['arap_iters_run']}; oracle stop-rule ratios {so['ratio'].tolist()}; GPU - oracle energy "
           f"{(st['energy'][:5] - so['energy'][:5]).tolist()} (oracle {so['energy'][:5].tolist()})")
    assert st["n_valid"] == so["n_valid"] and st["arap_iters_run"] == so["arap_iters_run"], why
    if rtol is not None:
        assert np.allclose(st["energy"][:5], so["energy"][:5], rtol=rtol, atol=1e-12), why
    return float((np.abs(st["energy"][:5] - so["energy"][:5]) / np.maximum(np.abs(so["energy"][:5]), 1e-300)).max())


def stop_ratios(so):
    """``so`` (oracle Deform.iterate) with its stop-rule ratios |E(t-1)-E(t)|/E(t) added as ``ratio``"""
    e = so["energy"][:so["arap_iters_run"]]
    so["ratio"] = np.abs(np.diff(e)) / e[1:]
    return so


def check_batch(st, tol, n=None):
    """health of a batch: every solve judged on the device, none above cg_tol, ``n`` outer iterations done"""
    assert st["status"] == 0 and st["unconverged_solves"] == 0 and st["worst_rel_residual_in_batch"] <= tol, st
    assert n is None or st["outer_done"] == n, st


def check_state(d, v_ref, rot_ref, tag):
    """vertices and per-vertex rotations of handle ``d`` within 1e-6 RMS of the oracle's -> (vertex RMS, rotation RMS)"""
    dv, dr = rms(d.vertices(), v_ref), rms(d.rotations().reshape(-1, 9), np.reshape(rot_ref, (-1, 9)))
    assert dv <= 1e-6 and dr <= 1e-6, (tag, dv, dr)
    return dv, dr
