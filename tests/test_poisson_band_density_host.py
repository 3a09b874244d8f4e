"""Host side of mvs_poisson_reconstruct_band_density (include/mvs.h, rules 32-35): the symbols; the refusals that come before a device
is needed; PoissonFiles' routing; on the restatement tests/ref_poisson_band_density.py the conditions that keep the scenes of
tests/poisson_band_density_scenes.py from testing nothing — gains that span a range and are cut, a weighted right-hand side and mesh
that differ from the unweighted ones, inactive blocks, vertices whose density cell has a corner without storage, a face equality that
is well posed — and what the weighting achieves at a band depth; and rule 32's read (csrc/poisson_band_rules.h) with the bytes of the
density structure (csrc/poisson_band_plan.h) as a stand-alone program under the address and undefined-behaviour sanitizers, against
values the restatement wrote to a file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import poisson_band_density_calls as CALLS, poisson_band_density_scenes as S, poisson_density_scenes as DS
from tests import ref_poisson as R, ref_poisson_band as RB, ref_poisson_band_density as RBD, ref_poisson_density as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = CALLS.E_INVALID, CALLS.E_NO_DEVICE


def test_symbols_and_python_forms():
    lib = C.CDLL(L.LIB_PATH)
    for name in CALLS.FORMS + ("mvs_processor_poisson_band_density", "mvs_test_poisson_band_density_level"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert callable(P.RunPoissonBandDensity) and lib.mvs_abi_version() == 4
    assert C.sizeof(L.CPoissonBandInfo) == 424 and C.sizeof(L.CPoissonDensityInfo) == 32      # the structs of the two calls, unchanged


@pytest.mark.parametrize("fn", CALLS.FORMS)
@pytest.mark.parametrize("kw", CALLS.BAD, ids=[CALLS.ident(kw) for kw in CALLS.BAD])
def test_refusals_need_no_device(kw, fn):
    assert CALLS.call(fn=fn, **kw) == E_INVALID
    assert fn.encode() in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    """the host form only: with a device present the call runs, and the arrays of CALLS.call are host arrays"""
    ok = (0, E_NO_DEVICE) if L.device_count() else (E_NO_DEVICE,)
    assert CALLS.call() in ok
    assert CALLS.call(density=False) in ok                                  # vertex_density may be NULL
    assert CALLS.call(dfields=dict(max_gain=16.0, density_drop=8, flags=1), depth_min=10, depth_max=10, scale=1.04) in ok
    assert CALLS.call(dfields=dict(max_gain=1.0, density_drop=0), bfields=dict(base_depth=3, band=64)) in ok


def test_the_hook_and_the_file_entry_check_their_arguments_too(tmp_path):
    buf, ci, bi, di, p = np.zeros((8, 3)), L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo(), P.poisson_params()
    bp, dp, bad_dp = P.poisson_band_params(), P.poisson_density_params(), P.poisson_density_params(density_drop=9)
    small, small8, sums = np.zeros(8), np.zeros(8, np.uint8), np.zeros(8, np.int64)
    lib = L.lib()

    def hook(dparams, dinfo, rho):
        return lib.mvs_test_poisson_band_density_level(4, L.ptr(buf), L.ptr(buf), C.byref(p), C.byref(bp), dparams, C.byref(ci), C.byref(bi), dinfo, 9,
                                                       L.ptr(small8), L.ptr(small8), L.ptr(small), L.ptr(small), 8, L.ptr(sums), 8, rho, L.ptr(small))

    assert hook(C.byref(bad_dp), C.byref(di), L.ptr(small)) == E_INVALID and b"density_drop" in lib.mvs_last_error()
    assert hook(None, C.byref(di), L.ptr(small)) == E_INVALID and hook(C.byref(dp), None, L.ptr(small)) == E_INVALID
    assert hook(C.byref(dp), C.byref(di), None) == E_INVALID and b"rho" in lib.mvs_last_error()
    dst = os.fsencode(str(tmp_path / "m.obj"))
    assert lib.mvs_processor_poisson_band_density(None, C.byref(p), C.byref(bp), C.byref(dp), 0.0, dst, None, None, None) == E_INVALID
    assert lib.mvs_processor_poisson_band_density(dst, C.byref(p), C.byref(bp), C.byref(dp), float("nan"), dst, None, None, None) == E_INVALID
    assert b"trim_ratio" in lib.mvs_last_error() and not os.path.exists(dst)


def test_poisson_files_routes_bparams_with_dparams_and_trim_ratio_and_still_refuses_sparams(tmp_path):
    src, dst = str(tmp_path / "none.npts"), str(tmp_path / "m.obj")
    for kw in (dict(dparams=P.poisson_density_params(), trim_ratio=0.0), dict(dparams=P.poisson_density_params(flags=1), trim_ratio=0.25)):
        with pytest.raises(L.MvsError) as e:                                # no such file, or no device: the new entry was reached
            P.PoissonFiles(src, dst, bparams=P.poisson_band_params(), **kw)
        assert e.value.code != E_INVALID and "bparams" not in str(e.value)
    # dparams and trim_ratio go together; one without the other raises as before (tests/test_poisson_band_entry_host.py)
    for kw in (dict(sparams=P.poisson_screen_params()), dict(sparams=P.poisson_screen_params(), dparams=P.poisson_density_params(), trim_ratio=0.5),
               dict(dparams=P.poisson_density_params()), dict(trim_ratio=0.5)):
        with pytest.raises(L.MvsError) as e:
            P.PoissonFiles(src, dst, bparams=P.poisson_band_params(), **kw)
        assert e.value.code == E_INVALID and "bparams" in str(e.value)
    assert not os.path.exists(dst)


# ------------------------------------------------------------------ the scenes ----
@pytest.mark.parametrize("name", S.UNEVEN6)
def test_the_uneven_scenes_weight_something(name):
    """measured: gains 0.41-4.0, 0.52-4.0, 0.30-4.0; 297, 237, 200 rows cut; on uneven6 30 077 of the 124 638 free nodes of level 6 have
    a non-zero b, weighted or not, and the two differ at every one of them"""
    w, u = S.reference(name, True), S.reference(name, False)
    assert w["depth"] == 6 and w["base_depth"] == 4 and w["density_depth"] == S.DENSITY_DEPTHS[name]
    assert w["gain"].min() <= 0.6 and w["gain"].max() >= 3.0 and w["n_clamped"] > 0
    assert w["gain"].tobytes() == u["gain"].tobytes() and w["node_sums"].tobytes() == u["node_sums"].tobytes()
    D = w["depth"]
    free = w["levels"][D]["cls"] == RB.FREE
    bw, bu = w["levels"][D]["b"], u["levels"][D]["b"]
    some = free & ((bw != 0.0) | (bu != 0.0))
    print(f"{name}: gain {w['gain'].min():.2f} .. {w['gain'].max():.2f}, {w['n_clamped']} cut; b differs at {int((bw != bu)[some].sum())} of the {int(some.sum())} "
          f"free nodes of level {D} where it is not zero ({int(free.sum())} free)")
    assert some.sum() > 1000 and (bw != bu)[some].all()
    assert np.array_equal(w["levels"][D]["act"], u["levels"][D]["act"])       # rule 33: the blocks depend on the positions only
    assert not np.array_equal(w["faces"], u["faces"])


@pytest.mark.parametrize("name", S.SIX)
def test_every_band_level_leaves_blocks_inactive(name):
    ref = S.reference(name, True)
    assert sorted(ref["levels"]) == [5, 6]
    for l, lv in ref["levels"].items():
        assert 0 < lv["n_active"] < lv["act"].size and not lv["act"].all(), (name, l)


@pytest.mark.parametrize("name", ("uneven6", "open6"))
def test_vertices_read_nodes_without_storage(name):
    """Dd = 5 > B = 4: block storage.  Measured: 3696 resp. 5513 vertices of the weighted mesh have a density cell with a corner of sum
    0, and some of those corners lie in blocks that are not stored — the zero of rule 32 is read, and it is exact: no node outside the
    stored blocks has a sum"""
    ref = S.reference(name, True)
    assert ref["density_depth"] == 5 > ref["base_depth"]
    corner = RBD.corner_sums(ref["vertices"], ref["node_sums"], ref["origin"], ref["hd"], ref["Gd"])
    stored_blocks, stored = RBD.stored_nodes(ref["P"], ref["origin"], ref["side"], ref["density_depth"])
    S3 = ref["node_sums"].reshape(stored.shape)
    assert (S3[~stored] == 0).all() and (S3 != 0).any()
    i0, _ = R.corners_weights(ref["vertices"], ref["origin"], ref["hd"], ref["Gd"])
    unstored = np.zeros(len(i0), bool)
    for c in range(8):
        unstored |= ~stored[i0[:, 2] + (c >> 2 & 1), i0[:, 1] + (c >> 1 & 1), i0[:, 0] + (c & 1)]
    print(f"{name}: {int((corner == 0).any(1).sum())} of {len(corner)} vertices with a corner of sum 0, {int(unstored.sum())} with a corner that is not stored; "
          f"{int(stored_blocks.sum())} of {stored_blocks.size} blocks stored")
    assert (corner == 0).any(1).sum() >= 1 and unstored.sum() >= 1 and not stored_blocks.all()


CASES = [(n, True) for n in S.SIX + ("all_active5",)] + [("uneven6", False)]


@pytest.mark.parametrize("name,weight", CASES, ids=[f"{n}-{'weighted' if w else 'plain'}" for n, w in CASES])
def test_face_equality_is_well_posed(name, weight):
    """as tests/test_poisson_band_entry_host.py: every node of level D that has a value clears iso by more than 2 (E_dev + E_ref), and the
    gap of RB.extract exceeds 1e-6 (smallest measured: 8.3e-6, uneven6 unweighted), so the vertex bound B of the GPU test is finite"""
    ref = S.reference(name, weight)
    E_dev = RB.accumulated_bound(ref, lambda l, lv: S.TOL)
    E_ref = RB.accumulated_bound(ref, lambda l, lv: lv["rel"] if "rel" in lv else lv["rel_residual"])
    chi = ref["chi"]
    margin = float(np.abs(chi[~np.isnan(chi)] - ref["iso"]).min())
    print(f"{name} {'weighted' if weight else 'plain'}: min |chi - iso| {margin:.2e} against 2 (E_dev + E_ref) {2.0 * (E_dev + E_ref):.2e}; gap {ref['gap']:.2e}")
    assert margin > 2.0 * (E_dev + E_ref)
    assert ref["gap"] > 1e-6 and ref["gap"] - 2.0 * (E_dev + E_ref) > 0.0


def test_the_gap_of_the_dense_scene():
    for weight in (False, True):
        assert S.reference("at_base", weight)["gap"] > 1e-6


def test_open_edges_of_the_open_scene():
    """measured: 256 open edges weighted, 268 unweighted"""
    w, u = S.reference("open6", True), S.reference("open6", False)
    print(f"open6: open edges {w['n_open_edges']} weighted, {u['n_open_edges']} unweighted")
    assert w["n_open_edges"] > 0 and u["n_open_edges"] > 0
    kept, kf = RD.trim(len(w["vertices"]), w["faces"], w["vertex_density"], S.TRIM_RATIO * w["rho_mean"])
    assert 0 < len(kept) < len(w["vertices"]) and 0 < len(kf) < len(w["faces"])


def test_what_the_weighting_achieves_at_a_band_depth():
    """uneven6 from the restatement.  Measured: radial rms 1.311 h unweighted, 0.074 h weighted (17.7 x)"""
    w, u = S.reference("uneven6", True), S.reference("uneven6", False)
    rw, ru = RD.radial_rms(w["vertices"], (0, 0, 0), 1.0, w["h"]), RD.radial_rms(u["vertices"], (0, 0, 0), 1.0, u["h"])
    print(f"uneven6: radial rms {ru[0]:.4f} h (max {ru[1]:.3f} h, V {len(u['vertices'])}) unweighted, {rw[0]:.4f} h (max {rw[1]:.3f} h, V {len(w['vertices'])}) weighted")
    assert rw[0] <= 0.1 and rw[0] <= 0.1 * ru[0]


def test_with_every_block_active_the_restatement_is_the_dense_density_call():
    """all_active5 against tests/ref_poisson_density.py on the same points at depth 5: the density, and b at the free nodes"""
    ref, dense = S.reference("all_active5", True), DS.reference("uneven", True)
    assert ref["depth"] == dense["depth"] == 5 and ref["density_depth"] == dense["density_depth"] == 4 and ref["levels"][5]["act"].all()
    for key in ("node_sums", "rho", "gain"):
        assert ref[key].tobytes() == dense[key].tobytes(), key
    assert ref["rho_mean"] == dense["rho_mean"] and ref["n_clamped"] == dense["n_clamped"]
    free = ref["levels"][5]["cls"] == RB.FREE
    assert ref["levels"][5]["b"][free].tobytes() == dense["rhs"][free].tobytes() and np.array_equal(ref["faces"], dense["faces"])
    base = S.reference("at_base", True)
    assert "levels" not in base and base["vertices"].tobytes() == dense["vertices"].tobytes() and base["faces"].tobytes() == dense["faces"].tobytes()


# ------------------------------------------------------------------ the rules header as a program ----
def _block_storage(ref):
    """the restatement's dense sums in the library's storage -> (T, num [T^3] int32, sums [64 ns] int64)"""
    stored_blocks, _ = RBD.stored_nodes(ref["P"], ref["origin"], ref["side"], ref["density_depth"])
    T, n1 = stored_blocks.shape[0], ref["Gd"] + 1
    num = np.full(T ** 3, -1, np.int32)
    where = np.flatnonzero(stored_blocks.reshape(-1))                       # (bz, by, bx) order
    num[where] = np.arange(len(where), dtype=np.int32)
    padded = np.zeros((4 * T,) * 3, np.int64)
    padded[:n1, :n1, :n1] = ref["node_sums"].reshape(n1, n1, n1)
    blocks = padded.reshape(T, 4, T, 4, T, 4).transpose(0, 2, 4, 1, 3, 5).reshape(T ** 3, 64)      # [block][lz, ly, lx]
    return T, num, np.ascontiguousarray(blocks[where]).reshape(-1)


def test_the_read_of_rule_32_under_the_sanitizers(tmp_path):
    """tests/poisson_band_density_rules.cpp: a stand-alone program, nothing is preloaded.  Its own cases; then the vertices and the
    points of two scenes read through a block table built from the restatement — among them vertices whose cell has corners that are
    not stored — equal RD.density_at on the dense sums bit for bit."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "poisson_band_density_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "poisson_band_density_rules.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "poisson band density rules ok" in run.stdout, run.stdout + run.stderr
    for name in ("uneven6", "open6"):
        ref = S.reference(name, True)
        T, num, sums = _block_storage(ref)
        rows = np.concatenate([ref["vertices"], ref["P"]])
        fin, fout = str(tmp_path / f"{name}.in"), str(tmp_path / f"{name}.out")
        with open(fin, "wb") as fh:
            fh.write(np.asarray(list(ref["origin"]) + [ref["hd"]], np.float64).tobytes())
            fh.write(np.asarray([ref["Gd"], T, len(sums) // 64, len(rows)], np.int32).tobytes())
            fh.write(num.tobytes())
            fh.write(sums.tobytes())
            fh.write(np.ascontiguousarray(rows, np.float64).tobytes())
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        got = np.fromfile(fout, np.float64)
        want = RD.density_at(rows, ref["node_sums"], ref["origin"], ref["hd"], ref["Gd"])
        assert len(got) == len(rows) and got.tobytes() == want.tobytes(), name
        assert got[:len(ref["vertices"])].tobytes() == ref["vertex_density"].tobytes() and got[len(ref["vertices"]):].tobytes() == ref["rho"].tobytes()
        assert (num == -1).any() and len(sums) // 64 < T ** 3
