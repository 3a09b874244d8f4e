"""The band levels of the Poisson stage without a GPU: the restatement tests/ref_poisson_band.py (rules 24-31, stated in
csrc/poisson_band_rules.h) against tests/ref_poisson.py where the two must agree, the conditions that keep a scene from silently
testing the dense case, rule 31 against the boundary of the mesh, and csrc/poisson_band_rules.h, run as a host program of its own
(tests/poisson_band_rules.cpp), against the restatement's blocks, node classes, edge states and start values."""
import os
import subprocess

import numpy as np
import pytest

from tests import poisson_band_scenes as BS, ref_poisson as R, ref_poisson_band as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0))


def test_with_every_block_active_the_restatement_is_the_dense_one():
    pts, nrm, prm, _ = BS.scene("all_active")
    ref, dense = BS.reference("all_active"), R.reconstruct(pts, nrm, **prm)
    top = ref["levels"][5]
    assert ref["depth"] == dense["depth"] == 5 and top["act"].all() and ref["h"] == dense["h"]
    inner = (slice(1, -1),) * 3
    assert (top["cls"][inner] == RB.FREE).all() and top["b"][inner].tobytes() == dense["rhs"][inner].tobytes()
    # the band solve of level 5 stands on fixed values 0 (the boundary of the grid): the same system, two solves
    E = R.stop_bound(top["rel"], dense["rhs"], 5) + R.stop_bound(dense["rel_residual"], dense["rhs"], 5)
    diff = float(np.abs(top["chi"] - dense["chi"]).max())
    print(f"all_active: max |chi_band - chi_dense| {diff:.2e} against {E:.2e}")
    assert diff <= E and abs(ref["iso"] - dense["iso"]) <= E
    assert np.array_equal(ref["faces"], dense["faces"]) and ref["n_open_edges"] == 0
    assert float(np.abs(ref["vertices"] - dense["vertices"]).max()) <= 1e-10 * ref["h"]


def test_at_or_below_the_base_depth_the_restatement_is_the_dense_one():
    pts, nrm, prm, bprm = BS.scene("at_base")
    ref, dense = BS.reference("at_base"), R.reconstruct(pts, nrm, **prm)
    assert ref["depth"] == 4 <= bprm["base_depth"] and "levels" not in ref
    assert ref["vertices"].tobytes() == dense["vertices"].tobytes() and ref["faces"].tobytes() == dense["faces"].tobytes() and ref["iso"] == dense["iso"]


def test_depth_max_above_10_means_10():
    P = np.random.default_rng(3).normal(size=(50, 3))
    o, side = R.cube_of(P, 1.3)
    prm = dict(R.DEFAULTS, depth_min=3, samples_per_node=1e-9)             # every candidate depth qualifies
    assert RB.pick_depth(P, o, side, dict(prm, depth_max=12)) == RB.pick_depth(P, o, side, dict(prm, depth_max=10)) == 10
    assert R.pick_depth(P, o, side, dict(prm, depth_max=12)) == 9


@pytest.mark.parametrize("name", BS.PARITY)
def test_scene_conditions(name):
    """rule 26's nesting at every level; at every band level a block that is not active, and free nodes beside fixed ones in each of
    the six directions: the scene tests a band, not the dense grid"""
    ref = BS.reference(name)
    cover = None
    for l in sorted(ref["levels"]):
        lv = ref["levels"][l]
        act, cls = lv["act"], lv["cls"]
        if cover is not None:
            assert cover.repeat(2, 0).repeat(2, 1).repeat(2, 2)[act].all()
        cover = act
        if name == "hemisphere" and l == 4:                                 # base 3: level 4 is 4^3 blocks and band 1 reaches them all
            assert act.all()
            continue
        assert not act.all() and lv["n_active"] == int(act.sum()) and lv["n_free"] == int((cls == RB.FREE).sum())
        n1 = cls.shape[0]
        for dz, dy, dx in SHIFTS:
            a = cls[max(dz, 0):n1 + min(dz, 0), max(dy, 0):n1 + min(dy, 0), max(dx, 0):n1 + min(dx, 0)]
            b = cls[max(-dz, 0):n1 + min(-dz, 0), max(-dy, 0):n1 + min(-dy, 0), max(-dx, 0):n1 + min(-dx, 0)]
            assert ((a == RB.FREE) & (b == RB.FIXED)).any(), (name, l, (dz, dy, dx))
        assert not np.isnan(lv["chi"][cls != RB.NONE]).any() and np.isnan(lv["chi"][cls == RB.NONE]).all()
        assert lv["rel"] <= 1e-13


def test_properties_of_the_band_meshes():
    """closed where the band holds the whole surface, two components for the two bands, and — rule 31 — open where the surface leaves
    the band: every boundary edge of the mesh joins two vertices on counted edges.  The hemisphere at base 3 -> D 5, band 1 stays
    closed (n_open_edges = 0, V 4402, F 8800): the low points of the dome keep the blocks under it active, so the closure of the scan
    stays inside the band; the cap z > 0.5 at base 4 -> D 6 is the scene whose closure leaves it (n_open_edges = 316)."""
    for name, comps_want, euler_want in (("two_levels", 1, 2), ("two_spheres", 2, 4), ("clipped", 1, 2), ("hemisphere", 1, 2)):
        ref = BS.reference(name)
        closed, euler, comps, vol = R.mesh_properties(ref["vertices"], ref["faces"])
        assert closed and comps == comps_want and euler == euler_want and vol > 0.0 and ref["n_open_edges"] == 0, name
    from scipy import ndimage
    act = BS.reference("two_spheres")["levels"][6]["act"]
    assert ndimage.label(act, structure=np.ones((3, 3, 3)))[1] == 2
    top = BS.reference("clipped")["levels"][6]
    edge = np.ones(top["cls"].shape, bool)
    edge[1:-1, 1:-1, 1:-1] = False
    assert (top["cls"][edge] == RB.FIXED).any() and (top["cls"][edge] != RB.FREE).all() and (top["chi"][edge & (top["cls"] == RB.FIXED)] == 0.0).all()
    ref = BS.reference("cap")
    f, nv = ref["faces"].astype(np.int64), len(ref["vertices"])
    und = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, inv, cnt = np.unique(und[:, 0] * nv + und[:, 1], return_inverse=True, return_counts=True)
    boundary = und[cnt[inv.reshape(-1)] == 1]
    print(f"cap: V {nv} F {len(f)} open edges {ref['n_open_edges']} boundary edges of the mesh {len(boundary)}")
    assert ref["n_open_edges"] == int(ref["open_vertex"].sum()) > 0 and len(boundary) > 0 and ref["open_vertex"][boundary].all()


def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "poisson_band_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "poisson_band_rules.cpp"), "-o", exe])
    return exe


def test_the_shared_rules_agree_with_the_restatement(tmp_path):
    """csrc/poisson_band_rules.h as a host program: the order of the rows on block sets of its own; then, for a band level of four
    scenes, the active blocks, the node classes, `exists` and `open` of every edge and the start values, all exactly the restatement's"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "poisson band rules ok" in run.stdout, run.stdout + run.stderr
    for name, l in (("two_levels", 5), ("clipped", 6), ("hemisphere", 5), ("cap", 5)):
        _, _, _, bprm = BS.scene(name)
        ref = BS.reference(name)
        lv = ref["levels"][l]
        below = ref["levels"][l - 1]["chi"] if l - 1 in ref["levels"] else ref["base"]["chi"]
        G, n1 = lv["G"], lv["G"] + 1
        fin, fout = str(tmp_path / f"{name}.in"), str(tmp_path / f"{name}.out")
        with open(fin, "wb") as fh:
            fh.write(np.asarray(list(ref["origin"]) + [ref["side"]], np.float64).tobytes())
            fh.write(np.asarray([l, bprm["band"], len(ref["P"]), 0], np.int32).tobytes())
            fh.write(np.ascontiguousarray(ref["P"], np.float64).tobytes())
            fh.write(np.ascontiguousarray(below, np.float64).tobytes())
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = open(fout, "rb").read()
        gb, nn = G // 4, n1 ** 3
        assert len(raw) == gb ** 3 + nn + 14 * nn + 8 * nn
        blocks = np.frombuffer(raw, np.uint8, gb ** 3).reshape(gb, gb, gb)
        cls = np.frombuffer(raw, np.uint8, nn, gb ** 3).reshape(n1, n1, n1)
        assert np.array_equal(blocks, lv["act"].astype(np.uint8)) and np.array_equal(cls, lv["cls"]), name
        pad = np.pad(lv["cell"], 1)
        for t, (dx, dy, dz) in enumerate(R.ETYPE):
            ex = np.frombuffer(raw, np.uint8, nn, gb ** 3 + nn + 2 * t * nn).reshape(n1, n1, n1)
            op = np.frombuffer(raw, np.uint8, nn, gb ** 3 + nn + (2 * t + 1) * nn).reshape(n1, n1, n1)
            want_ex, want_op = np.zeros((n1, n1, n1), np.uint8), np.zeros((n1, n1, n1), np.uint8)
            want_ex[:n1 - dz, :n1 - dy, :n1 - dx], want_op[:n1 - dz, :n1 - dy, :n1 - dx] = RB.edge_cells(pad, n1, (dx, dy, dz))
            assert np.array_equal(ex, want_ex) and np.array_equal(op, want_op), (name, t)
        start = np.frombuffer(raw, np.float64, nn, gb ** 3 + 15 * nn).reshape(n1, n1, n1)
        want = RB.start_values(below)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(start), nan) and start[~nan].tobytes() == want[~nan].tobytes(), name
