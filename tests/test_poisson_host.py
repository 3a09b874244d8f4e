"""Host side of mvs_poisson_reconstruct (include/mvs.h): symbols, the layouts of mvs_poisson_params and mvs_poisson_info, the argument
checks (they run before a device is needed), properties of the numpy / scipy restatement tests/ref_poisson.py on the scenes of
tests/poisson_scenes.py, the conditions those scenes must meet for the GPU comparison to be exact, and the shared rules header
(csrc/poisson_rules.h) as a stand-alone program under the address and undefined-behaviour sanitizers, on its own cases and against tables
dumped from the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import poisson_scenes as SC, ref_poisson as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -4


def _call(n=4, points=True, normals=True, prm=True, info=True, vertices=True, faces=True, vcap=8, fcap=8, **fields):
    pts, nrm = np.zeros((4, 3)), np.zeros((4, 3))
    pts[:, 0] = np.arange(4)
    v, f, ci = np.zeros((8, 3)), np.zeros((8, 3), np.int32), L.CPoissonInfo()
    p = P.poisson_params(**fields)
    return L.lib().mvs_poisson_reconstruct(n, L.ptr(pts) if points else None, L.ptr(nrm) if normals else None, C.byref(p) if prm else None,
                                           C.byref(ci) if info else None, L.ptr(v) if vertices else None, vcap, L.ptr(f) if faces else None, fcap)


def test_symbols_layouts_and_defaults():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_poisson_default_params", "mvs_poisson_reconstruct", "mvs_poisson_reconstruct_dev", "mvs_processor_poisson",
                 "mvs_test_poisson_field"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T, I = L.CPoissonParams, L.CPoissonInfo
    assert C.sizeof(T) == 40 and T.samples_per_node.offset == 8 and T.solve_tol.offset == 16 and T.depth_max.offset == 24
    assert T.depth_min.offset == 28 and T.max_cycles.offset == 32 and T.reserved.offset == 36
    assert C.sizeof(I) == 80 and I.h.offset == 24 and I.iso.offset == 32 and I.rel_residual.offset == 40 and I.n_used.offset == 48
    assert I.n_vertices.offset == 56 and I.n_faces.offset == 64 and I.depth.offset == 72 and I.cycles.offset == 76
    p = P.poisson_params()
    assert (p.scale, p.samples_per_node, p.solve_tol, p.depth_max, p.depth_min, p.max_cycles, p.reserved) == (1.1, 1.5, 1e-8, 10, 7, 64, 0)
    assert lib.mvs_abi_version() == 4
    with pytest.raises(L.MvsError):
        P.poisson_params(depth=8)


BAD = [dict(points=False), dict(normals=False), dict(prm=False), dict(info=False), dict(vertices=False), dict(faces=False), dict(n=-1),
       dict(scale=math.nan), dict(scale=math.inf), dict(scale=0.0), dict(scale=-1.1), dict(samples_per_node=math.nan), dict(samples_per_node=0.0),
       dict(samples_per_node=-1.5), dict(samples_per_node=math.inf), dict(solve_tol=math.nan), dict(solve_tol=0.0), dict(solve_tol=-1e-8),
       dict(solve_tol=math.inf), dict(scale=1.03125), dict(scale=1.5, depth_min=3, depth_max=3), dict(scale=1.25, depth_min=4),
       dict(depth_min=2, scale=4.0), dict(depth_min=8, depth_max=7), dict(depth_min=10, depth_max=10), dict(max_cycles=0), dict(max_cycles=-3),
       dict(vcap=-1), dict(fcap=-1)]


def _id(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BAD, ids=[_id(kw) for kw in BAD])
def test_argument_errors_need_no_device(kw):
    assert _call(**kw) == E_INVALID
    assert b"mvs_poisson_reconstruct" in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    ok = (0, E_NO_DEVICE) if L.device_count() else (E_NO_DEVICE,)
    assert _call() in ok
    assert _call(scale=1.04) in ok                                          # 1 + 4 / 2^7 = 1.03125 is the first scale refused
    assert _call(scale=1.51, depth_min=3, depth_max=3) in ok
    assert _call(scale=1.51, depth_min=3, depth_max=2 ** 31 - 1, max_cycles=2 ** 31 - 1) in ok
    assert _call(vertices=False, faces=False, vcap=0, fcap=0) in ok + (E_INVALID,)         # sizes a second call: -1 only after the counts


def test_the_device_form_the_hook_and_the_file_entry_check_their_arguments_too(tmp_path):
    buf, ci, p = np.zeros((8, 3)), L.CPoissonInfo(), P.poisson_params(max_cycles=0)
    assert L.lib().mvs_poisson_reconstruct_dev(4, L.ptr(buf), L.ptr(buf), C.byref(p), C.byref(ci), L.ptr(buf), 8, L.ptr(buf), 8, None) == E_INVALID
    assert b"mvs_poisson_reconstruct_dev" in L.lib().mvs_last_error()
    assert L.lib().mvs_test_poisson_field(4, L.ptr(buf), L.ptr(buf), C.byref(p), C.byref(ci), L.ptr(buf), L.ptr(buf), 8) == E_INVALID
    assert L.lib().mvs_processor_poisson(None, C.byref(p), os.fsencode(str(tmp_path / "m.obj")), None, None) == E_INVALID
    if L.device_count() == 0:
        with pytest.raises(L.MvsError) as e:
            P.PoissonFiles(str(tmp_path / "none.npts"), str(tmp_path / "m.obj"))
        assert e.value.code == E_NO_DEVICE and not (tmp_path / "m.obj").exists()


@pytest.mark.parametrize("name", SC.NAMES)
def test_properties_of_the_restatement(name):
    ref = SC.reference(name)
    assert ref["depth"] == SC.DEPTHS[name] and len(ref["vertices"]) > 100
    closed, euler, comps, vol = R.mesh_properties(ref["vertices"], ref["faces"])
    assert closed                                                          # every directed edge once, its reverse once
    assert comps == SC.COMPONENTS[name] and euler == 2 * comps
    assert vol > 0.0                                                       # wound outward
    f = ref["faces"]
    assert f.min() == 0 and f.max() == len(ref["vertices"]) - 1 and (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()     # rotated: smallest first
    if name == "sphere":
        assert abs(vol - 4.0 / 3.0 * math.pi) <= 0.015 * 4.0 / 3.0 * math.pi
        rad = np.sqrt(((ref["vertices"] - np.array([0.3, -0.2, 1.7])) ** 2).sum(1))
        assert np.abs(rad - 1.0).max() <= 0.6 * ref["h"]
    if name == "ellipsoid":
        assert abs(vol - 4.0 / 3.0 * math.pi * 0.35) <= 0.015 * 4.0 / 3.0 * math.pi * 0.35


@pytest.mark.parametrize("name", SC.NAMES)
def test_scene_conditions(name):
    """what makes the GPU comparison at solve_tol = 1e-12 exact: with E = solve_tol |b| / lambda_min the bound on what the stopping rule
    can move any chi value, and iso, by — no inside decision can move (every node clears iso by 100 * 2E), rule 3's choice is not within
    1 % of its threshold at any candidate depth, and the bound B on the movement of a vertex is at most 1e-4 h"""
    pts, nrm, prm = SC.scene(name)
    ref = SC.reference(name)
    D, h = ref["depth"], ref["h"]
    E = R.stop_bound(SC.TOL, ref["rhs"], D)
    margin = float(np.abs(ref["chi"] - ref["iso"]).min())
    B = math.sqrt(3.0) * h * 4.0 * E / (ref["gap"] - 2.0 * E)
    print(f"{name}: D {D} E {E:.2e} node margin {margin:.2e} ({margin / (200.0 * E):.0f} x 200 E) B {B / h:.2e} h direct-solve residual {ref['rel_residual']:.1e}")
    assert margin >= 100.0 * 2.0 * E
    assert ref["gap"] > 2.0 * E and B <= 1e-4 * h
    assert ref["rel_residual"] <= 1e-13
    full = dict(R.DEFAULTS, **prm)
    for d in range(full["depth_min"], min(full["depth_max"], R.MAX_DEPTH) + 1):
        need = full["samples_per_node"] * R.occupied(ref["P"], ref["origin"], ref["side"], d)
        assert abs(ref["n_used"] - need) > 0.01 * need
    if name == "picked":
        assert full["depth_min"] < D < full["depth_max"]


def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "poisson_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "poisson_rules.cpp"), "-o", exe])
    return exe


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """tests/poisson_rules.cpp: the edge-type and Kuhn tables, clamped cells, ties of the quantisation, points on the faces of the cube;
    then the header against the restatement: corners, weights and quantised contributions of the ellipsoid scene's points (plus the two
    corners of the cube) bit for bit, and the triangles of all 14 mixed inside patterns of each of the six tetrahedra"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "poisson rules ok" in run.stdout, run.stdout + run.stderr
    pts, nrm, _ = SC.scene("ellipsoid")
    ref = SC.reference("ellipsoid")
    o, h, G = ref["origin"], ref["h"], ref["G"]
    Pp = np.concatenate([pts[:400], [o, o + ref["side"]]])
    Nn = np.concatenate([nrm[:400], [[1.0, -1.0, 0.5], [-0.25, 1.0, 1.0]]])
    rng = np.random.default_rng(5)
    val = np.concatenate([-rng.uniform(0.05, 2.0, 8), rng.uniform(0.05, 2.0, 8)])          # corner values when inside / when outside, iso = 0
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.asarray(list(o) + [h], np.float64).tobytes())
        fh.write(np.asarray([G, len(Pp)], np.int32).tobytes())
        fh.write(np.concatenate([Pp, Nn], 1).astype(np.float64).tobytes())
        fh.write(val.tobytes())
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    rec = np.dtype([("i0", "<i4", (4,)), ("w", "<f8", (8,)), ("q", "<i8", (8, 3))])
    got = np.frombuffer(raw[:rec.itemsize * len(Pp)], rec)
    i0, w = R.corners_weights(Pp, o, h, G)
    assert np.array_equal(got["i0"][:, :3], i0) and i0.min() == 0 and i0.max() == G - 1
    assert got["w"].tobytes() == np.stack(w, 1).tobytes()
    want_q = np.stack([np.stack([np.rint((w[c] * Nn[:, a]) * R.Q).astype(np.int64) for a in range(3)], 1) for c in range(8)], 1)
    assert np.array_equal(got["q"], want_q)
    table = np.frombuffer(raw[rec.itemsize * len(Pp):], np.int32).reshape(6, 14, 5)
    for k in range(6):
        corners = R.tet_corners(k)
        for pattern in range(1, 15):
            ins = [bool(pattern >> i & 1) for i in range(4)]
            cyc, d = R.tet_cycle(corners, ins)
            idx, pos = [], []
            for i, j in cyc:
                idx.append(R.edge_key((0, 0, 0), corners, i, j, 2))
                mi, mo = sum(corners[i][a] << a for a in range(3)), sum(corners[j][a] << a for a in range(3))
                a, b = float(val[mi]), float(val[8 + mo])
                t = (0.0 - a) / (b - a)
                pos.append(tuple(float(corners[i][q]) + t * (float(corners[j][q]) - float(corners[i][q])) for q in range(3)))
            want = R.polygon(idx, pos, d)
            assert table[k, pattern - 1, 0] == len(want) and table[k, pattern - 1, 1:1 + len(want)].tolist() == want
            assert (table[k, pattern - 1, 1 + len(want):] == -1).all()
