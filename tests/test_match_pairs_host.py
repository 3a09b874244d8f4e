"""Host side of the sequence-pair entries (include/mvs.h mvs_match_filter(_pairs(_dev)), mvs_sequence_pair_srt): the symbols, the
layout of mvs_seq_pair_params, the argument checks, which run before any device is needed, and the host code the entries share
(csrc/frontend_dev.h mp_stage1, csrc/engine.h check_offsets) as a stand-alone program under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from multiviewstitch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -4
W, H, VIEWS, N1, N2 = 8, 6, 2, 2, 1


def test_the_three_symbols_are_exported():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("mvs_match_filter_pairs", "mvs_match_filter_pairs_dev", "mvs_sequence_pair_srt"):
        assert hasattr(lib, name) and name in _lib.EXPORTS


def test_seq_pair_params_layout_matches_the_header():
    src = open(os.path.join(ROOT, "include", "mvs.h")).read()
    body = re.search(r"typedef struct mvs_seq_pair_params \{(.*?)\} mvs_seq_pair_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"mvs_match_filter_params": C.sizeof(_lib.CMatchFilterParams), "double": 8, "int32_t": 4}
    fields = []                                                  # (type, name) in declaration order
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [(words[0], w) for w in words[1:]]
    assert [n for _, n in fields] == [n for n, _ in _lib.CSeqPairParams._fields_]
    off = 0
    for (ty, name), (_, cty) in zip(fields, _lib.CSeqPairParams._fields_):
        assert C.sizeof(cty) == size[ty]
        off = (off + min(8, size[ty]) - 1) // min(8, size[ty]) * min(8, size[ty])     # natural alignment, as the C compiler lays it out
        assert getattr(_lib.CSeqPairParams, name).offset == off, name
        off += size[ty]
    assert C.sizeof(_lib.CSeqPairParams) == (off + 7) // 8 * 8 == 72
    assert C.sizeof(_lib.CMatchFilterParams) == 32


def _args():
    npx = W * H
    a = dict(n1=N1, n2=N2, off=np.array([0, 2, 3], np.int64), raw=np.zeros((3, 6), np.int32),
             tex1=np.zeros((N1, VIEWS, npx), np.int32), valid1=np.ones((N1, npx), np.uint8), tex2=np.zeros((N2, VIEWS, npx), np.int32),
             valid2=np.ones((N2, npx), np.uint8), imgs1=np.zeros((N1, H, W, 3), np.uint8), imgs2=np.zeros((N2, H, W, 3), np.uint8),
             prm=_lib.CMatchFilterParams(W, H, VIEWS, 1, 6.0, 2, 0), out=np.zeros((3, 4), np.int32), ooff=np.zeros(N1 * N2 + 1, np.int64),
             cnt=np.zeros((N1 * N2, 3), np.int64))
    return a


def _filter_call(dev, **kw):
    a = _args()
    a.update(kw)
    P = _lib.ptr
    prm = C.byref(a["prm"]) if a["prm"] is not None else None
    common = (a["n1"], a["n2"], P(a["off"]), P(a["raw"]), P(a["tex1"]), P(a["valid1"]), P(a["tex2"]), P(a["valid2"]), P(a["imgs1"]), P(a["imgs2"]),
              prm, P(a["out"]), P(a["ooff"]), P(a["cnt"]))
    L = _lib.lib()
    return L.mvs_match_filter_pairs_dev(*common, None) if dev else L.mvs_match_filter_pairs(*common)


BAD_OFFSETS = [np.array([1, 2, 3], np.int64), np.array([0, 3, 2], np.int64)]


def test_match_filter_pairs_rejects_bad_arguments_without_a_device():
    wide = _lib.CMatchFilterParams(65536, H, VIEWS, 1, 6.0, 2, 0)
    tall = _lib.CMatchFilterParams(W, 65536, VIEWS, 1, 6.0, 2, 0)
    cases = [dict(off=None), dict(raw=None), dict(tex1=None), dict(valid1=None), dict(tex2=None), dict(valid2=None), dict(imgs1=None),
             dict(imgs2=None), dict(prm=None), dict(out=None), dict(ooff=None), dict(off=BAD_OFFSETS[0]), dict(off=BAD_OFFSETS[1]),
             dict(prm=wide), dict(prm=tall), dict(n1=0), dict(n1=-1), dict(n2=0),
             dict(prm=_lib.CMatchFilterParams(W, H, 0, 1, 6.0, 2, 0)), dict(prm=_lib.CMatchFilterParams(W, H, VIEWS, -1, 6.0, 2, 0))]
    for dev in (False, True):
        for kw in cases:
            assert _filter_call(dev, **kw) == E_INVALID, (dev, kw)
            assert _lib.lib().mvs_last_error()
        assert _filter_call(dev, cnt=None) != E_INVALID             # stage_counts is optional (no device: MVS_E_NO_DEVICE)


def _srt_call(**kw):
    from multiviewstitch_amd import scene as S
    a = _args()
    cam = S.Camera(10.0, 10.0, W / 2 - 0.5, H / 2 - 0.5, np.eye(3), np.zeros(3), W, H)
    a.update(cams1=(_lib.CCamera * N1)(*[_lib.CCamera.of(cam)] * N1), cams2=(_lib.CCamera * N2)(*[_lib.CCamera.of(cam)] * N2),
             d1=np.full((N1, H * W), 0.1, np.float32), d2=np.full((N2, H * W), 0.1, np.float32),
             sp=_lib.CSeqPairParams(a["prm"], 0.0025, 0.3, 7, 200, 60.0, 0.75), st=C.c_uint32(1), f1=C.c_int32(), f2=C.c_int32(),
             s=C.c_double(), R=np.zeros(9), t=np.zeros(3))
    a.update(kw)
    P = _lib.ptr
    ref = lambda x: C.cast(C.byref(x), C.c_void_p) if x is not None else None
    return _lib.lib().mvs_sequence_pair_srt(a["n1"], a["n2"], ref(a["cams1"]), ref(a["cams2"]), P(a["d1"]), P(a["d2"]), P(a["off"]), P(a["raw"]),
                                            P(a["tex1"]), P(a["tex2"]), P(a["imgs1"]), P(a["imgs2"]), ref(a["sp"]), ref(a["st"]), ref(a["f1"]),
                                            ref(a["f2"]), ref(a["s"]), P(a["R"]), P(a["t"]), None, None, None, None, None, None)


def test_sequence_pair_srt_rejects_bad_arguments_without_a_device():
    prm = _args()["prm"]
    wide = _lib.CSeqPairParams(_lib.CMatchFilterParams(65536, H, VIEWS, 1, 6.0, 2, 0), 0.0025, 0.3, 7, 200, 60.0, 0.75)
    no_iters = _lib.CSeqPairParams(prm, 0.0025, 0.3, 7, 0, 60.0, 0.75)
    other_size = _lib.CSeqPairParams(_lib.CMatchFilterParams(W + 1, H, VIEWS, 1, 6.0, 2, 0), 0.0025, 0.3, 7, 200, 60.0, 0.75)
    for kw in [dict(cams1=None), dict(cams2=None), dict(d1=None), dict(d2=None), dict(off=None), dict(raw=None), dict(tex1=None), dict(tex2=None),
               dict(imgs1=None), dict(imgs2=None), dict(sp=None), dict(st=None), dict(f1=None), dict(f2=None), dict(s=None), dict(R=None),
               dict(t=None), dict(off=BAD_OFFSETS[0]), dict(off=BAD_OFFSETS[1]), dict(sp=wide), dict(sp=no_iters), dict(sp=other_size),
               dict(n1=0), dict(n2=-3)]:
        assert _srt_call(**kw) == E_INVALID, kw
        assert _lib.lib().mvs_last_error()
    assert _srt_call() != E_INVALID                                  # every optional output NULL


def _one_pair_call(**kw):
    npx = W * H
    a = dict(raw=np.zeros((3, 6), np.int32), tex1=np.zeros((VIEWS, npx), np.int32), valid1=np.ones(npx, np.uint8),
             tex2=np.zeros((VIEWS, npx), np.int32), valid2=np.ones(npx, np.uint8), img1=np.zeros((H, W, 3), np.uint8),
             img2=np.zeros((H, W, 3), np.uint8), prm=_lib.CMatchFilterParams(W, H, VIEWS, 1, 6.0, 2, 0), out=np.zeros((3, 4), np.int32),
             n_out=C.c_int64(-7), cnt=np.zeros(3, np.int64))
    a.update(kw)
    P = _lib.ptr
    rc = _lib.lib().mvs_match_filter(P(a["raw"]), len(a["raw"]), P(a["tex1"]), P(a["valid1"]), P(a["tex2"]), P(a["valid2"]), P(a["img1"]),
                                     P(a["img2"]), C.byref(a["prm"]), P(a["out"]), C.byref(a["n_out"]), P(a["cnt"]))
    return rc, a["n_out"].value


def test_match_filter_checks_arguments_then_view_indices_then_the_device():
    """the order mvs_match_filter keeps: bad arguments, then a view index out of range, then the missing device"""
    for kw in [dict(tex1=None), dict(valid1=None), dict(tex2=None), dict(valid2=None), dict(img1=None), dict(img2=None), dict(out=None),
               dict(prm=_lib.CMatchFilterParams(65536, H, VIEWS, 1, 6.0, 2, 0)), dict(prm=_lib.CMatchFilterParams(W, 65536, VIEWS, 1, 6.0, 2, 0))]:
        assert _one_pair_call(**kw) == (E_INVALID, -7), kw
        assert _lib.lib().mvs_last_error()
    bad_view = np.zeros((3, 6), np.int32)
    bad_view[2, 0] = VIEWS                                           # view1 = view_count, everything else valid
    assert _one_pair_call(raw=bad_view) == (E_INVALID, -7)
    assert b"view index out of range" in _lib.lib().mvs_last_error()
    if _lib.device_count() == 0:
        assert _one_pair_call() == (E_NO_DEVICE, -7)
    else:                                                            # (the suite on a GPU machine: the three matches are one key, at a border)
        assert _one_pair_call() == (0, 0)


def test_the_shared_host_rules_under_the_sanitizers(tmp_path):
    """tests/frontend_rules.cpp: mp_stage1 at the edge pixels and at tex = -1, check_offsets on an empty list, a descending pair and
    the limit value — host code, compiled without the device pass and run as a program of its own"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "frontend_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "frontend_rules.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "frontend rules ok" in run.stdout, run.stdout + run.stderr
