"""The deformation solvers on meshes with vertices of valence 9 .. 40 (tests/mesh_valence.py; every other mesh of the suite has
valence <= 8): the passes > 1 loops of the local step (local_dev.h, also inside the fused last launch of a patch solve), the
row loops over r.passes of the weight / right-hand-side / SpMV kernels and cg_gather_tail (arap.hip), the patch tables at width
12 and 16 (meshbuild.hip, schwarz.hip), MVS_SOLVER_AUTO falling back to CG above valence 16, and real edges of weight exactly 0
(the kernels' padding sentinel) in a second pass.

Tolerances are the project's (mesh_valence.tolerances): energies rtol 1e-6, vertex and rotation RMS 1e-7 x extent at cg_tol 1e-10.
The two CPU references differ by ~1e-14 on every case (tests/test_valence_meshes.py), so no case needs a wider figure.
"""
import functools

import numpy as np
import pytest

from multiviewstitch_amd import scene as S
from tests import mesh_sheets as MS, mesh_valence as MV
from tests.util import check_batch, check_pass, check_state, rms, stop_ratios

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from multiviewstitch_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    from multiviewstitch_amd import deformation
    return deformation


@functools.lru_cache(maxsize=None)
def _reference(name, hubs_in):
    """nodes, targets and oracle.arap of a case: computed once, shared by both solvers"""
    from oracle import binding as O
    m = MV.case(name)
    nodes = MV.nodes_of(m, O, hubs_in)
    tg = MV.target_field(m.pts[nodes])
    ref = O.arap(m.pts, m.faces, nodes, tg, 5, 1e-4)
    for a in (nodes, tg, *ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return nodes, tg, ref


def _assert_solver(d, m, solver):
    info = d.solver_info()
    kind, width = m.expect
    if solver == 1:
        assert info["kind"] == "cg", info
    else:
        assert info["kind"] == kind, (m.name, info)                # valence > 16 or V < 2048: AUTO is CG
        if kind == "patch":
            assert info["width"] == width, (m.name, info)


@pytest.mark.parametrize("hubs_in", [True, False])
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("name", MV.CASES)
def test_arap_matches_oracle(eng, name, solver, hubs_in):
    """(a), (e): every case under both solvers, every hub once a Dirichlet row and once a free row.  d12_obtuse: four real edges
    of a hub, row positions 8..11, have weight exactly 0.0 — they must change neither the iteration count nor the energies."""
    m = MV.case(name)
    nodes, tg, ref = _reference(name, hubs_in)
    d = eng.Deformation(m.pts, m.normals, m.faces)
    d.params.solver = solver
    d.params.cg_tol = 1e-10
    _assert_solver(d, m, solver)
    d.set_nodes(nodes)
    st = d.arap(tg)
    n = ref["iters"]
    e_rtol, v_tol, r_tol = MV.tolerances(name, hubs_in)
    de = float((np.abs(st["energy"][:n] - ref["energies"][:n]) / ref["energies"][:n]).max())
    dv = rms(d.vertices(), ref["pts"]) / m.extent
    dr = rms(d.rotations().reshape(-1, 9), ref["rot"].reshape(-1, 9))
    print(f"[measured] {name} solver={solver} hubs_in={hubs_in}: iters {st['arap_iters_run']}/{n} energy rel {de:.2e} (tol {e_rtol:.0e}) "
          f"vertex RMS/extent {dv:.2e} (tol {v_tol:.0e}) rotation RMS {dr:.2e} (tol {r_tol:.0e}) residual {st['cg_rel_residual']:.2e}")
    assert st["arap_iters_run"] == n
    assert st["status"] == 0 and st["cg_rel_residual"] <= 1.5 * d.params.cg_tol
    assert np.allclose(st["energy"][:n], ref["energies"][:n], rtol=e_rtol, atol=0)
    assert dv <= v_tol and dr <= r_tol, (dv, dr)
    d.close()


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("name", MV.CASES)
def test_known_answers(eng, oracle, name, solver):
    """(b): answers that do not pass through the oracle.  Targets = the rest pose: the rest pose comes back to 1e-10, R_i = I to
    1e-9.  Targets = one rigid motion of all nodes: every rotation is that motion's to 1e-9 and the energy is at most 1e-18 x
    extent^2.  The rigid motion is a translation: started from R_i = I, as CGAL's deform() and the engine start, the local /
    global iteration reproduces a rigid motion exactly only when its rotation is the identity — with a rotation by 0.3 rad even
    the exact CPU oracle is 5e-3 off after its five iterations (5e-8 after fifty), so no bound of 1e-9 can be asked of that."""
    m = MV.case(name)
    nodes = MV.nodes_of(m, oracle, False)

    def handle():
        # one handle per answer, as test_arap_matches_oracle_and_known_answers: a handle sizes the launch plan of a solve from
        # its previous ones (mvs.h), and the rest pose's solve, which needs no iteration at all, says nothing about the next
        d = eng.Deformation(m.pts, m.normals, m.faces)
        d.params.solver = solver
        d.params.cg_tol = 1e-12
        _assert_solver(d, m, solver)
        d.set_nodes(nodes)
        return d

    d = handle()
    st = d.arap(m.pts[nodes])
    dv, dr = np.abs(d.vertices() - m.pts).max(), np.abs(d.rotations() - np.eye(3)).max()
    print(f"[measured] {name} solver={solver} rest pose: vertices {dv:.2e} rotations {dr:.2e}")
    assert st["status"] == 0 and dv <= 1e-10 and dr <= 1e-9
    d.close()
    t = np.array([0.1, -0.2, 0.05])
    d = handle()
    st = d.arap(m.pts[nodes] + t)
    n = st["arap_iters_run"]
    dv, dr, e = np.abs(d.vertices() - (m.pts + t)).max(), np.abs(d.rotations() - np.eye(3)).max(), float(np.abs(st["energy"][:n]).max())
    print(f"[measured] {name} solver={solver} translation: vertices {dv:.2e} rotations {dr:.2e} energy {e:.2e} (bound {1e-18 * m.extent ** 2:.2e})")
    assert st["status"] == 0 and dr <= 1e-9 and dv <= 1e-9
    assert e <= 1e-18 * m.extent ** 2
    d.close()


@functools.lru_cache(maxsize=None)
def _scan():
    """a scan for the full pass: a denser sphere on the same surface, slightly swollen and bent"""
    dirs, faces = S.geodesic_sphere(24)
    p = MV.surface(dirs) * (1.02 + 0.02 * np.sin(3 * dirs[:, 2:3]))
    p[:, 0] += 0.03 * dirs[:, 2] ** 2
    n = S.vertex_normals_plyobj(p, faces)
    p.setflags(write=False)
    n.setflags(write=False)
    return p, n


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("name", ["d12", "d16"])
def test_full_pass_matches_oracle(eng, oracle, name, solver):
    """(c): set_target plus three iterate(1) against oracle.Deform, as test_iterate_matches_oracle; then one iterate(4) on a fresh
    handle.  On a patch solve the rotations come from the fused last launch: the passes > 1 path of local_dev.h inside schwarz.hip."""
    m = MV.case(name)
    tp, tn = _scan()
    nodes = MV.nodes_of(m, oracle, False)
    p = oracle.Params.default()

    def pair():
        d = eng.Deformation(m.pts, m.normals, m.faces)
        d.params.solver = solver
        _assert_solver(d, m, solver)
        d.set_nodes(nodes)
        d.set_target(tp, tn)
        o = oracle.Deform(m.pts, m.normals, m.faces)
        o.set_nodes(nodes)
        o.set_target(tp, tn)
        return d, o

    d, o = pair()
    for it in range(3):
        st, so = d.iterate(1), o.iterate(p, 1)
        assert st["arap_iters_run"] == so["arap_iters_run"] and st["n_valid"] == so["n_valid"] and so["n_valid"] > len(nodes) // 4
        assert np.allclose(st["energy"][:5], so["energy"][:5], rtol=1e-6, atol=1e-12)
        assert st["cg_rel_residual"] <= 1.5 * d.params.cg_tol
        dv, dr = rms(d.vertices(), o.vertices()), rms(d.rotations().reshape(-1, 9), o.rotations().reshape(-1, 9))
        print(f"[measured] {name} solver={solver} outer {it}: vertex RMS {dv:.2e} rotation RMS {dr:.2e}")
        assert dv <= 1e-6 and dr <= 1e-6, f"outer {it}"
    d.close()
    d, o = pair()
    st, so = d.iterate(4), stop_ratios(o.iterate(p, 4))
    de = check_pass(st, so, f"{name} iterate(4)", 1e-6)
    check_batch(st, d.params.cg_tol, 4)
    dv, dr = check_state(d, o.vertices(), o.rotations(), f"{name} iterate(4)")
    print(f"[measured] {name} solver={solver} iterate(4): energy rel {de:.2e} vertex RMS {dv:.2e} rotation RMS {dr:.2e}")
    d.close()


def test_results_are_bit_reproducible_on_d16(eng, oracle):
    """(d): two fresh handles give identical bytes; the patch solver and the CG agree to the solve tolerance (each ends within
    cg_tol of the same systems: 1e-7 on the vertices, as test_a_handle_is_reused_for_the_next_fit)."""
    m = MV.case("d16")
    tp, tn = _scan()
    outs = []
    for solver in (0, 0, 1):
        d = eng.Deformation(m.pts, m.normals, m.faces)
        d.params.solver = solver
        _assert_solver(d, m, solver)
        d.UniformSampling(16)
        d.set_target(tp, tn)
        d.iterate(1)
        st = d.iterate(2)
        assert st["status"] == 0
        outs.append((d.vertices(), d.rotations(), np.array(st["energy"])))
        d.close()
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    dv, dr = rms(outs[0][0], outs[2][0]), rms(outs[0][1].reshape(-1, 9), outs[2][1].reshape(-1, 9))
    print(f"[measured] d16 patch solver against CG: vertex RMS {dv:.2e} rotation RMS {dr:.2e}")
    assert dv <= 1e-7 * m.extent and dr <= 1e-6
    assert np.allclose(outs[0][2][:5], outs[2][2][:5], rtol=1e-6, atol=1e-12)


# ---- flat sheets (tests/mesh_sheets.py): every covariance of the local step has rank 2 — exactly (z = 0) or to rounding (tilted) ----
@functools.lru_cache(maxsize=None)
def _sheet_reference(name):
    from oracle import binding as O
    m = MS.case(name)
    ref = O.arap(m.pts, m.faces, m.nodes, m.targets, 5, 1e-4)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("name", MS.CASES)
def test_arap_on_flat_sheets(eng, name, solver):
    """As test_arap_matches_oracle (cg_tol 1e-10), on meshes whose 1-rings are flat (about 7 % of the real edge weights are exactly
    0.0 as well, test_sheet_is_what_it_says); and every rotation is a proper rotation about the plane's normal n: |R n - n| <= 1e-12.

    A rotation keeps n as well as its 1-ring lies in the plane: it tilts by (off-plane error of the vertices) / (edge length, 0.05).
    On the axis-aligned sheets z stays exactly 0 and the bound holds at any solve tolerance.  On the tilted ones the vertices are
    off the plane by what the linear solve leaves: measured at cg_tol 1e-10, 1e-12, 1e-13, 1e-14 the worst |R n - n| was 1.0e-9,
    2.8e-11, 2.8e-12, 3.3e-13 (large_tilted, CG) — proportional to the tolerance, nothing of the SVD's.  The oracle's direct solve
    leaves 6.7e-13 on that sheet.  The bound is therefore asserted on a second solve at cg_tol 1e-14, which every case reaches
    (residuals <= 6e-15), and that solve is compared with the oracle as well."""
    from tests import rotation_cases as RC
    m = MS.case(name)
    ref = _sheet_reference(name)
    n = ref["iters"]
    be, bv, br = MS.CPU_DISAGREEMENT[name]
    e_rtol, v_tol, r_tol = max(MV.E_RTOL, 10 * be), max(MV.RMS_TOL, 10 * bv), max(MV.RMS_TOL, 10 * br)
    det_tol = RC.GPU_FACTOR * RC.ORACLE_WORST["det"]
    for cg_tol in (1e-10, 1e-14):
        d = eng.Deformation(m.pts, m.normals, m.faces)
        d.params.solver = solver
        d.params.cg_tol = cg_tol
        _assert_solver(d, m, solver)
        d.set_nodes(m.nodes)
        st = d.arap(m.targets)
        R = d.rotations()
        de = float((np.abs(st["energy"][:n] - ref["energies"][:n]) / ref["energies"][:n]).max())
        dv = rms(d.vertices(), ref["pts"]) / m.extent
        dr = rms(R.reshape(-1, 9), ref["rot"].reshape(-1, 9))
        rn = float(np.abs(R @ m.n - m.n).max())
        det = float(np.abs(np.linalg.det(R) - 1).max())
        normal_kept = name.endswith("_flat") or cg_tol == 1e-14
        print(f"[measured] {name} solver={solver} cg_tol={cg_tol:.0e}: iters {st['arap_iters_run']}/{n} energy rel {de:.2e} (tol {e_rtol:.0e}) "
              f"vertex RMS/extent {dv:.2e} (tol {v_tol:.0e}) rotation RMS {dr:.2e} (tol {r_tol:.0e}) residual {st['cg_rel_residual']:.2e} "
              f"|R n - n| {rn:.2e} ({'bound 1e-12' if normal_kept else 'not asserted at this tolerance'}) |det R - 1| {det:.2e} (bound {det_tol:.1e})")
        assert st["arap_iters_run"] == n
        assert st["status"] == 0 and st["cg_rel_residual"] <= 1.5 * cg_tol
        assert np.allclose(st["energy"][:n], ref["energies"][:n], rtol=e_rtol, atol=0)
        assert dv <= v_tol and dr <= r_tol, (dv, dr)
        assert np.isfinite(R).all() and det <= det_tol, det
        if normal_kept:
            assert rn <= 1e-12, rn
        d.close()
