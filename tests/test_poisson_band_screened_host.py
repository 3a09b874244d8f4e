"""Host side of mvs_poisson_reconstruct_band_screened (include/mvs.h, rules 36-41): the struct, the symbols, the ABI version; the
refusals that come before a device is needed; PoissonBandScreenedFiles' routing; the byte plan (csrc/poisson_band_plan.h) as a
stand-alone program under the address and undefined-behaviour sanitizers against a count made array by array and against the
restatement's own block and row counts; and on the restatement tests/ref_poisson_band_screened.py what keeps the scenes of
tests/poisson_band_screened_scenes.py from testing nothing: a stencil that is exactly symmetric, alpha = 0 the band-density
restatement byte for byte, every touched node FREE (rule 38's argument), the cells of `block_corners`, a face equality that is well
posed, and what screening achieves at a band depth."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import poisson_band_density_scenes as DS, poisson_band_screened_scenes as S
from tests import ref_poisson as R, ref_poisson_band as RB, ref_poisson_band_density as RBD, ref_poisson_band_screened as RBS, ref_poisson_density as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -4
MESH_SCENES = ("two_levels", "clipped", "cap", "uneven6")


def test_struct_symbols_and_abi():
    lib = C.CDLL(L.LIB_PATH)
    for name in S.FORMS + ("mvs_processor_poisson_band_screened", "mvs_test_poisson_band_screened_level"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert callable(P.RunPoissonBandScreened) and callable(P.PoissonBandScreenedFiles) and lib.mvs_abi_version() == 4
    T = L.CPoissonBandScreenInfo
    assert C.sizeof(T) == 4 * 11 * 8 == 352
    assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, _ in T._fields_] == [("lambda_", 0, 88), ("target", 88, 88), ("occupied", 176, 88),
                                                                                      ("active_nodes", 264, 88)]
    # the structs of the calls it is made of, unchanged
    assert C.sizeof(L.CPoissonBandInfo) == 424 and C.sizeof(L.CPoissonScreenInfo) == 56 and C.sizeof(L.CPoissonDensityInfo) == 32
    assert C.sizeof(L.CPoissonInfo) == 80


def ident(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


@pytest.mark.parametrize("fn", S.FORMS)
@pytest.mark.parametrize("kw", S.BAD, ids=[ident(kw) for kw in S.BAD])
def test_refusals_need_no_device(kw, fn):
    assert S.call(fn=fn, **kw) == E_INVALID
    assert fn.encode() in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    """the host form only: with a device present the call runs, and the arrays of S.call are host arrays"""
    ok = (0, E_NO_DEVICE) if L.device_count() else (E_NO_DEVICE,)
    assert S.call() in ok
    assert S.call(density=False) in ok                                      # vertex_density may be NULL
    assert S.call(sfields=dict(alpha=0.0)) in ok and S.call(sfields=dict(alpha=64.0), bfields=dict(base_depth=3, band=64)) in ok


def test_the_hook_and_the_file_entry_check_their_arguments_too(tmp_path):
    buf, p, bp, dp, sp = np.zeros((8, 3)), P.poisson_params(), P.poisson_band_params(), P.poisson_density_params(), P.poisson_screen_params()
    ci, bi, di, si, bsi = L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo(), L.CPoissonScreenInfo(), L.CPoissonBandScreenInfo()
    small, small8, sums, st = np.zeros(8), np.zeros(8, np.uint8), np.zeros(8, np.int64), np.zeros(8 * 27, np.int64)
    bad_sp = P.poisson_screen_params(alpha=65.0)
    lib = L.lib()

    def hook(sparams=C.byref(sp), sinfo=C.byref(si), bsinfo=C.byref(bsi), stencil=L.ptr(st), f=L.ptr(small), start=L.ptr(small)):
        return lib.mvs_test_poisson_band_screened_level(4, L.ptr(buf), L.ptr(buf), C.byref(p), C.byref(bp), C.byref(dp), C.byref(ci), C.byref(bi), C.byref(di), 9,
                                                        L.ptr(small8), L.ptr(small8), L.ptr(small), L.ptr(small), 8, L.ptr(sums), 8, L.ptr(small), L.ptr(small),
                                                        sparams, sinfo, bsinfo, stencil, f, start)

    assert hook(sparams=C.byref(bad_sp)) == E_INVALID and b"alpha" in lib.mvs_last_error()
    assert hook(sparams=None) == E_INVALID and hook(sinfo=None) == E_INVALID
    assert hook(bsinfo=None) == E_INVALID and b"bsinfo" in lib.mvs_last_error()
    for kw in (dict(stencil=None), dict(f=None), dict(start=None)):
        assert hook(**kw) == E_INVALID and b"stencil" in lib.mvs_last_error()
    dst = os.fsencode(str(tmp_path / "m.obj"))
    assert lib.mvs_processor_poisson_band_screened(None, C.byref(p), C.byref(bp), C.byref(dp), C.byref(sp), 0.0, dst, None, None, None) == E_INVALID
    assert lib.mvs_processor_poisson_band_screened(dst, C.byref(p), C.byref(bp), C.byref(dp), C.byref(sp), float("nan"), dst, None, None, None) == E_INVALID
    assert b"trim_ratio" in lib.mvs_last_error() and not os.path.exists(dst)


def test_the_files_form_reaches_the_new_entry(tmp_path):
    src, dst = str(tmp_path / "none.npts"), str(tmp_path / "m.obj")
    for kw in (dict(), dict(params=P.poisson_params(), bparams=P.poisson_band_params(), dparams=P.poisson_density_params(flags=1),
                            sparams=P.poisson_screen_params(alpha=8.0), trim_ratio=0.25)):
        with pytest.raises(L.MvsError) as e:                                # no such file, or no device: the new entry was reached
            P.PoissonBandScreenedFiles(src, dst, **kw)
        assert e.value.code != E_INVALID
    with pytest.raises(L.MvsError) as e:
        P.PoissonBandScreenedFiles(src, dst, trim_ratio=float("nan"))
    assert e.value.code == E_INVALID and "mvs_processor_poisson_band_screened" in str(e.value)
    assert not os.path.exists(dst)


# ------------------------------------------------------------------ the byte plan as a program ----
def _stored_blocks(act):
    """k_bd_stored's rule on the restatement's active blocks: a block of the table (T = Gb + 1 per axis) is stored when it or its
    neighbour at offset -1 along any subset of the axes is active"""
    Gb = act.shape[0]
    T = Gb + 1
    stored = np.zeros((T, T, T), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                stored[dz:dz + Gb, dy:dy + Gb, dx:dx + Gb] |= act
    return int(stored.sum())


def test_the_byte_plan_under_the_sanitizers(tmp_path):
    """tests/poisson_band_screened_plan.cpp: a stand-alone program, nothing is preloaded.  Its own cases up to the extents of depth 10;
    then the level 6 of two scenes with the block and row counts of the restatement, against the bytes counted here array by array"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "poisson_band_screened_plan")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "poisson_band_screened_plan.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "poisson band screened plan ok" in run.stdout, run.stdout + run.stderr
    for name in ("uneven6", "block_corners"):
        ref = S.reference(name)
        lv = ref["levels"][6]
        stored, rows, used = _stored_blocks(lv["act"]), lv["active_nodes"], ref["n_used"]
        run = subprocess.run([exe, str(stored), str(rows), "6", str(used)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        nodes = 64 * stored
        nb = -(-nodes // 256)
        srows = -(-nb // 4096)
        want = [27 * 4 * stored + stored + 4 * nodes + 8 * nodes, 28 * 8 * rows + 4 * rows,
                nodes + 4 * nb + 4 * (nb + 1) + 4 * srows * 4097 + 4 * srows + 4 * (srows + 1), 2 ** 18 // 8, 8 * used]
        print(f"{name} level 6: {stored} stored blocks, {rows} rows, {used} used points -> {run.stdout.strip()}")
        assert [int(x) for x in run.stdout.split()] == want and 0 < rows < nodes


# ------------------------------------------------------------------ the restatement and its scenes ----
@pytest.mark.parametrize("name", S.LEVEL_SCENES)
def test_the_stencil_is_symmetric_and_every_touched_node_is_free(name):
    """rule 38 on every band level of every scene: S_{i,o} == S_{i+o,-o} as int64, the 27 neighbours of a node with a row all have a
    value, and every node a point touches is FREE"""
    ref = S.reference(name)
    for l, lv in ref["levels"].items():
        n1 = lv["G"] + 1
        St = lv["stencil"].reshape(n1, n1, n1, 27)
        cls = lv["cls"]
        touched = lv["touch"].reshape(n1, n1, n1) > 0
        assert touched.sum() == lv["active_nodes"] > 0 and (cls[touched] == RB.FREE).all(), (name, l)
        assert not St[~touched].any()
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    o, m = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), (1 - dz) * 9 + (1 - dy) * 3 + (1 - dx)
                    a = St[1:-1, 1:-1, 1:-1, o]
                    b = St[1 + dz:n1 - 1 + dz, 1 + dy:n1 - 1 + dy, 1 + dx:n1 - 1 + dx, m]
                    assert np.array_equal(a, b), (name, l, o)
                    has_value = cls[1 + dz:n1 - 1 + dz, 1 + dy:n1 - 1 + dy, 1 + dx:n1 - 1 + dx] != RB.NONE
                    assert has_value[touched[1:-1, 1:-1, 1:-1]].all(), (name, l, o)
        assert not touched[0].any() and not touched[-1].any() and not touched[:, 0].any() and not touched[:, -1].any()
        assert lv["lam"] == ref["alpha"] / max(1.0, ref["n_used"] / lv["occupied"])


@pytest.mark.parametrize("weight", (False, True), ids=("plain", "weighted"))
def test_alpha_zero_is_the_band_density_restatement(weight):
    pts, nrm, prm, bprm, dprm = DS.scene("uneven6")
    zero = RBS.reconstruct(pts, nrm, weight=weight, alpha=0.0, **bprm, **dprm, **prm)
    want = DS.reference("uneven6", weight)
    for key in ("vertices", "faces", "vertex_density", "chi", "node_sums", "rho", "gain"):
        assert zero[key].tobytes() == want[key].tobytes(), key
    assert zero["iso"] == want["iso"] and zero["n_open_edges"] == want["n_open_edges"]


def test_the_cells_of_block_corners():
    """every used point but the corner (1, 1, 1) lies in a level-6 cell whose index is 3 mod 4 on all three axes, one point per cell at
    most on levels 4, 5 and 6, so every lambda is alpha = 64; the two extreme cells of an axis add up to 63, which is why one point
    cannot have the property (tests/poisson_band_screened_scenes.py)"""
    pts, nrm, prm, bprm, dprm, alpha = S.scene("block_corners")
    ref = S.reference("block_corners")
    assert 300 <= len(pts) <= 600 and alpha == 64.0 and ref["depth"] == 6 and ref["base_depth"] == 4 and ref["n_used"] == len(pts)
    cells = R.cells_at(ref["P"], ref["origin"], ref["side"], 6)
    assert (cells[:-1] % 4 == 3).all() and cells[0].tolist() == [7, 7, 7] and cells[-1].tolist() == [56, 56, 56]
    assert (cells.min(0) + cells.max(0) == 63).all()
    for l in (4, 5, 6):
        assert R.occupied(ref["P"], ref["origin"], ref["side"], l) == len(pts), l
    assert ref["base"]["lam"] == 64.0 and ref["levels"][5]["lam"] == 64.0 and ref["levels"][6]["lam"] == 64.0
    # the eight corners of such a cell lie in eight different blocks: node indices 4 k + 3 and 4 k + 4 on every axis
    i0, _ = R.corners_weights(ref["P"][:-1], ref["origin"], ref["h"], 64)
    assert (i0 % 4 == 3).all() and ((i0 + 1) % 4 == 0).all()
    assert ref["levels"][6]["active_nodes"] == 8 * len(pts)                 # no two points share a corner


@pytest.mark.parametrize("name", MESH_SCENES)
def test_face_equality_is_well_posed(name):
    """every node of level D that has a value clears iso by more than twice the restatement's own uncertainty E_ref, and so does the gap
    of RB.extract: the restatement's faces are decided.  Whether a device run decides them the same way depends on the residuals it
    reaches — the bound is linear in them —, so the relative residual at which 2 (E_dev + E_ref) still stays below the margin is
    printed; the GPU test prints the margin beside the bound of the residuals it had.  Measured: the margin allows 7e-14 on two_levels"""
    ref = S.reference(name)
    E_tol = RBS.accumulated_bound(ref, S.TOL, S.TOL, lambda l: S.TOL)[0]
    E_ref = RBS.accumulated_bound(ref, ref["base"]["rel0"], ref["base"]["rel_residual"], lambda l: ref["levels"][l]["rel"])[0]
    chi = ref["chi"]
    margin = float(np.abs(chi[~np.isnan(chi)] - ref["iso"]).min())
    print(f"{name}: min |chi - iso| {margin:.2e}, gap {ref['gap']:.2e} against 2 E_ref {2.0 * E_ref:.2e}; E_dev with every solve at solve_tol {E_tol:.2e}: the "
          f"margin allows residuals of {S.TOL * (0.5 * margin - E_ref) / E_tol:.1e}; lmin {[round(lv['lmin'], 4) for lv in ref['levels'].values()]}")
    assert margin > 2.0 * E_ref and ref["gap"] > 2.0 * E_ref
    assert (ref["n_open_edges"] > 0) == (name == "cap")


def test_what_screening_achieves_at_a_band_depth():
    """uneven6 (the 4 : 1 sphere, depth 6 over base 4, band 1) without the weight flag: the radial rms of the screened mesh at alpha = 4
    is lower than the unscreened band's.  Measured: 1.311 h unscreened, 0.108 h screened (12.2 x); with the flag 0.074 h and 0.059 h"""
    pts, nrm, prm, bprm, dprm = DS.scene("uneven6")
    plain = DS.reference("uneven6", False)
    screened = RBS.reconstruct(pts, nrm, weight=False, alpha=4.0, **bprm, **dprm, **prm)
    ru = RD.radial_rms(plain["vertices"], (0, 0, 0), 1.0, plain["h"])
    rs = RD.radial_rms(screened["vertices"], (0, 0, 0), 1.0, screened["h"])
    rw = RD.radial_rms(S.reference("uneven6")["vertices"], (0, 0, 0), 1.0, screened["h"])
    print(f"uneven6: radial rms {ru[0]:.4f} h (max {ru[1]:.3f} h) unscreened, {rs[0]:.4f} h (max {rs[1]:.3f} h) screened at alpha 4: ratio {ru[0] / rs[0]:.2f}; "
          f"weighted and screened {rw[0]:.4f} h")
    assert abs(ru[0] - 1.311) < 1e-3 and rs[0] < ru[0]
