"""Host side of mvs_poisson_reconstruct_band (include/mvs.h, rules 24-31): on the restatement, that the face equality the GPU tests
ask for is well posed — no inside decision of a scene can move under the bounds of the two solves —; the symbols, layouts and defaults;
the refusals that come before a device is needed; PoissonFiles' refusal of bparams beside dparams; and csrc/poisson_band_plan.h, the
host's sizing and index arithmetic, as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import poisson_band_scenes as BS, ref_poisson_band as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -4


@pytest.mark.parametrize("name", ("all_active",) + BS.PARITY)
def test_face_equality_is_well_posed(name):
    """every node of level D that has a value clears iso by more than 2 (E_dev + E_ref): E_dev the accumulated bound with every solve
    stopped at TOL, E_ref the same bound at the restatement's own residuals.  Nothing may be left out: zero nodes.  Measured on the CPU:
    the smallest margin is 1.9e-7 (clipped) and 2.0e-7 (cap) against E_dev + E_ref <= 5.6e-10, and gap >= 1.9e-5, so B is finite."""
    ref = BS.reference(name)
    E_dev = RB.accumulated_bound(ref, lambda l, lv: BS.TOL)
    E_ref = RB.accumulated_bound(ref, lambda l, lv: lv["rel"] if "rel" in lv else lv["rel_residual"])
    chi = ref["chi"]
    margin = float(np.abs(chi[~np.isnan(chi)] - ref["iso"]).min())
    print(f"{name}: min |chi - iso| {margin:.2e} against 2 (E_dev + E_ref) {2.0 * (E_dev + E_ref):.2e}; gap {ref['gap']:.2e}")
    assert margin > 2.0 * (E_dev + E_ref)
    assert int((np.abs(chi[~np.isnan(chi)] - ref["iso"]) <= 2.0 * (E_dev + E_ref)).sum()) == 0
    assert ref["gap"] - 2.0 * (E_dev + E_ref) > 0.0


def test_symbols_layouts_and_defaults():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_poisson_band_default_params", "mvs_poisson_reconstruct_band", "mvs_poisson_reconstruct_band_dev", "mvs_processor_poisson_band",
                 "mvs_test_poisson_band_level"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T, I = L.CPoissonBandParams, L.CPoissonBandInfo
    assert C.sizeof(T) == 16 and T.band.offset == 4 and T.reserved.offset == 8
    assert I.n_free.offset == 88 and I.rel_residual.offset == 176 and I.bnorm.offset == 264 and I.iterations.offset == 352
    assert I.n_open_edges.offset == 400 and I.scratch_bytes.offset == 408 and I.base_depth.offset == 416 and I.failed_level.offset == 420 and C.sizeof(I) == 424
    bp = P.poisson_band_params()
    assert (bp.base_depth, bp.band, list(bp.reserved)) == (8, 2, [0, 0])
    assert P.poisson_band_params(band=3).band == 3
    with pytest.raises(L.MvsError):
        P.poisson_band_params(depth=8)


def _call(bparams=True, binfo=True, vcap=8, fcap=8, reserved=(0, 0), base_depth=8, band=2, **fields):
    # every array whose address goes into the call is bound to a name here and lives until the call has returned
    pts, nrm = np.zeros((4, 3)), np.zeros((4, 3))
    pts[:, 0] = np.arange(4)
    v, f, ci, bi = np.zeros((8, 3)), np.zeros((8, 3), np.int32), L.CPoissonInfo(), L.CPoissonBandInfo()
    p, bp = P.poisson_params(**fields), P.poisson_band_params(base_depth=base_depth, band=band)
    bp.reserved[0], bp.reserved[1] = reserved
    return L.lib().mvs_poisson_reconstruct_band(4, L.ptr(pts), L.ptr(nrm), C.byref(p), C.byref(bp) if bparams else None, C.byref(ci),
                                                C.byref(bi) if binfo else None, L.ptr(v), vcap, L.ptr(f), fcap)


BAD = [dict(bparams=False), dict(binfo=False), dict(base_depth=2), dict(base_depth=10), dict(band=0), dict(band=65), dict(reserved=(1, 0)),
       dict(reserved=(0, -1)), dict(depth_min=11, depth_max=11), dict(vcap=-1), dict(fcap=-1), dict(max_cycles=0), dict(scale=1.03125),
       dict(depth_min=8, depth_max=7)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD])
def test_refusals_need_no_device(kw):
    assert _call(**kw) == E_INVALID
    assert b"mvs_poisson_reconstruct_band" in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    ok = (0, E_NO_DEVICE) if L.device_count() else (E_NO_DEVICE,)
    assert _call() in ok
    assert _call(depth_min=10, depth_max=10, scale=1.04) in ok             # depth_min may reach 10 here
    assert _call(base_depth=3, band=64) in ok and _call(base_depth=9, band=1) in ok


def test_the_device_form_the_hook_and_the_file_entry_check_their_arguments_too(tmp_path):
    buf, ci, bi, p = np.zeros((8, 3)), L.CPoissonInfo(), L.CPoissonBandInfo(), P.poisson_params()
    bp = P.poisson_band_params(band=0)
    lib = L.lib()
    assert lib.mvs_poisson_reconstruct_band_dev(4, L.ptr(buf), L.ptr(buf), C.byref(p), C.byref(bp), C.byref(ci), C.byref(bi), L.ptr(buf), 8, L.ptr(buf), 8,
                                                None) == E_INVALID
    assert b"mvs_poisson_reconstruct_band_dev" in lib.mvs_last_error()
    small, small8 = np.zeros(8), np.zeros(8, np.uint8)
    assert lib.mvs_test_poisson_band_level(4, L.ptr(buf), L.ptr(buf), C.byref(p), C.byref(bp), C.byref(ci), C.byref(bi), 9, L.ptr(small8), L.ptr(small8),
                                           L.ptr(small), L.ptr(small), 8) == E_INVALID
    assert lib.mvs_processor_poisson_band(None, C.byref(p), C.byref(bp), os.fsencode(str(tmp_path / "m.obj")), None, None, None) == E_INVALID


def test_poisson_files_refuses_bparams_beside_the_density_and_screened_calls(tmp_path):
    src, dst = str(tmp_path / "none.npts"), str(tmp_path / "m.obj")
    for kw in (dict(dparams=P.poisson_density_params()), dict(sparams=P.poisson_screen_params()), dict(trim_ratio=0.5)):
        with pytest.raises(L.MvsError) as e:
            P.PoissonFiles(src, dst, bparams=P.poisson_band_params(), **kw)
        assert e.value.code == E_INVALID and "bparams" in str(e.value)
    assert not os.path.exists(dst)


def test_the_plan_header_under_the_sanitizers(tmp_path):
    """tests/poisson_band_plan.cpp: csrc/poisson_band_plan.h on an empty level, a full one, one stored block, blocks on the upper
    boundary of the grid and random sets, and at the extents of depth 10.  A stand-alone program: nothing is preloaded."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "poisson_band_plan")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "poisson_band_plan.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "poisson band plan ok" in run.stdout, run.stdout + run.stderr
