"""The coefficient cases of tests/jpeg_coef_cases.py without a GPU: the conditions that make them worth running (measured on the
restatement's unstuffed bytes, never on a kernel's), the reader's restatement tests/ref_jpeg.py against the writer's tests/ref_jpeg_enc.py
(two independent statements: what one wrote the other returns), the restatement's pixels against Pillow's (tests/golden/jpeg_coef; the
goldens against a fresh Pillow decode where Pillow is importable), the shared rules run as host programs of their own on the new inputs
(tests/jpeg_enc_rules.cpp on coefficient records, tests/jpeg_rules.cpp on the streams; plain, and under the address and
undefined-behaviour sanitizers), and the range checks of ``mvs_test_jpeg_encode_coef``.  Nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import jpeg_coef_cases as K, make_jpeg_coef_golden as G, ref_jpeg as R, ref_jpeg_enc as E
from tests import test_jpeg_enc_host as TE, test_jpeg_host as TD

FIX = G.load_all()
NAMES = list(K.CASES)
E_INVALID, E_NO_DEVICE = -1, -4
AC_SYMBOLS = {(r << 4) | s for r in range(16) for s in range(1, 11)}
E_BLOCK_BITS = 12 + 11 + 63 * (16 + 10)                              # JPEG_ENC_BLOCK_BITS of csrc/jpeg_enc_rules.h


def test_the_case_set_is_complete_and_the_goldens_small():
    """every mode with every kind, every restart form with ff and rand, every size; max has no golden"""
    cases = K.CASES.values()
    for kind in ("ff", "sym", "zrl", "rand", "max"):
        assert {c["mode"] for c in cases if c["kind"] == kind} == set(K.MODES), kind
    for kind in ("ff", "rand"):
        assert {c["restart"] for c in cases if c["kind"] == kind} == {0, 1, 2, K.ROW}, kind
    assert {(c["h"], c["w"]) for c in cases} == set(K.SIZES.values())
    long = K.CASES["long_75x100_444"]
    assert (long["h"], long["w"], long["mode"], long["restart"]) == (75, 100, "444", 0)
    assert sorted(FIX) == K.GOLDEN and not any(c["golden"] for c in cases if c["kind"] == "max")
    assert {K.CASES[n]["kind"] for n in K.GOLDEN} == {"ff", "sym", "zrl", "rand", "long"}
    for kind in ("ff", "sym", "zrl", "rand"):
        assert {K.CASES[n]["mode"] for n in K.GOLDEN if K.CASES[n]["kind"] == kind} == set(K.MODES), kind
    assert all(K.CASES[n]["quality"] == 100 for n in K.GOLDEN)
    size = sum(os.path.getsize(os.path.join(G.HERE, f)) for f in os.listdir(G.HERE))
    print(len(NAMES), "cases,", len(FIX), "goldens,", size, "bytes")
    assert size < 300 * 1024


def test_the_cases_reach_what_they_were_made_for():
    """from the restatement's unstuffed bytes and counters: FF-dense calls, runs of FF, FF in front of RSTn and of EOI, intervals across
    three stuffing chunks, chunks with several intervals, a segment of more than eight rings of the decoder, the longest block"""
    m = K.measure()
    for name, f in m.items():
        print(f"{name:26s} {f['bytes']:6d} bytes, {f['raw']:6d} unstuffed, FF {f['share']:.3f}, FF run {f['run']}, longest segment {f['segment']:6d}, "
              f"{f['intervals']:3d} intervals, longest block {f['bits']:4d} bits: {' '.join(sorted(f['carries']))}")
    carried = lambda what: [n for n, f in m.items() if what in f["carries"]]
    ff = [n for n in NAMES if K.CASES[n]["kind"] == "ff"]
    assert all(m[n]["share"] >= 0.5 for n in ff) and carried("half_ff") == ff
    assert carried("ff_run3") and max(f["run"] for f in m.values()) >= 3
    assert carried("ff_before_rst") and carried("ff_before_eoi")
    assert any(K.CASES[n]["kind"] == "rand" for n in carried("ff_before_rst")) and any(K.CASES[n]["kind"] == "max" for n in carried("ff_before_rst"))
    assert carried("interval_spans_3_chunks") and carried("chunk_holds_intervals")
    assert carried("segment_over_8_rings") == ["long_75x100_444"] and 26000 < m["long_75x100_444"]["raw"] < 28000
    assert m["long_75x100_444"]["intervals"] == 1
    mx = [n for n in NAMES if K.CASES[n]["kind"] == "max"]
    assert carried("block_1658_bits") == mx and max(f["bits"] for f in m.values()) == 1658 <= E_BLOCK_BITS
    assert all("zrl" in m[n]["carries"] for n in NAMES if K.CASES[n]["kind"] == "zrl")
    for n in NAMES:                                                  # one, two and three ZRLs in a row, a block without EOB, a block that is only EOB
        if K.CASES[n]["kind"] == "zrl" and (K.CASES[n]["h"], K.CASES[n]["w"]) == (33, 50):
            assert K.encoded(n)[2]["zrl"] >= 1 + 2 + 3 + 3 + 3, n


def test_the_chunk_boundary_call():
    """one call of several ``ff`` images: FF on both sides of a 1024-byte boundary of the call-wide unstuffed buffer (the carry of
    k_je_ffcount / k_je_stuff), and an FF in the last partial dword (the partial chunk of k_je_offsets)"""
    imgs, raw = K.boundary_call()
    both, tail = K.boundary_figures(raw)
    print(len(imgs), "images,", len(raw), "unstuffed bytes, FF on both sides of", both, ", total % 4 =", len(raw) % 4)
    assert len(imgs) >= 3 and both and tail and len(raw) > 3 * K.CHUNK


def test_every_symbol_of_both_tables_in_both_signs():
    """sym at 75x100 alone, in every mode: each of the 160 (run, size) symbols of the component's AC table with a positive and a negative
    value, ZRL and EOB; over all cases both signs of DC category 11 and category 0, in both tables"""
    for mode in K.MODES:
        seen = K.encoded(f"sym_75x100_{mode}")[3]
        for t in range(1 if mode == "grey" else 2):
            assert {s for s, _ in seen[t]["ac"]} == AC_SYMBOLS | {0x00, 0xF0}, (mode, t)
            assert all((s, True) in seen[t]["ac"] and (s, False) in seen[t]["ac"] for s in AC_SYMBOLS), (mode, t)
            assert {(11, True), (11, False), (0, None)} <= seen[t]["dc"], (mode, t)
    ac, dc = K.coverage()
    for t in range(2):
        assert len(ac[t]) == 2 * 160 + 2 and len(E.AC_CODES[t]) == 162
        assert {c for c, _ in dc[t]} == set(range(12))
    long16 = [sum(1 for s, (_, l) in E.AC_CODES[t].items() if l == 16) for t in range(2)]
    assert long16 == [125, 119]                                      # the codes past the decoder's 8-bit look-ahead, all of them produced


@pytest.mark.parametrize("name", NAMES)
def test_the_reader_returns_what_the_writer_was_given(name):
    """ref_jpeg.decode_all on ref_jpeg_enc.encode_coef's stream: the real blocks are exactly the case's, the dummy blocks hold no AC"""
    c = K.CASES[name]
    h, got, _, px = K.decoded(name)
    assert (h["w"], h["h"], len(h["segments"])) == (c["w"], c["h"], len(K.encoded(name)[1]))
    assert px.shape == (c["h"], c["w"], 3)
    for want, g, (pad, (rh, rw)) in zip(K.coef(name), got, K.geometry(c["h"], c["w"], c["mode"])):
        g = g.reshape(pad + (64,))
        assert np.array_equal(g[:rh, :rw], want[:rh, :rw])
        assert not g[rh:, :, 1:].any() and not g[:, rw:, 1:].any()     # a dummy block is a DC difference of 0 and EOB: no AC, the DC before it
        assert (want[rh:] == K.DUMMY).all() and (want[:, rw:] == K.DUMMY).all()


@pytest.mark.parametrize("name", K.GOLDEN)
def test_the_restatement_equals_pillow(name):
    data, px = FIX[name]
    assert data == K.encoded(name)[0]
    got = K.decoded(name)[3]
    print(name, len(data), "bytes,", int((got != px).sum()), "differing bytes")
    assert got.shape == px.shape and np.array_equal(got, px)
    assert np.array_equal(R.decode(data, "BGR"), px[..., ::-1])


def test_the_goldens_are_what_pillow_decodes_today():
    pytest.importorskip("PIL")
    fresh = G.fixtures()
    assert sorted(fresh) == sorted(FIX)
    for name, (data, px) in fresh.items():
        assert data == FIX[name][0], name
        px = np.stack([px] * 3, axis=2) if px.ndim == 2 else px
        assert np.array_equal(px, FIX[name][1]), name


# ------------------------------------------------------------------ the shared rules as programs ----
def _record(arrays, c):
    grey = c["mode"] == "grey"
    return (c["w"], c["h"], -1 if grey else -3, 0, c["quality"], 420 if grey else int(c["mode"]), c["restart"]), K.flat(arrays).tobytes()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_encoder_rules_on_coefficient_records(tmp_path, sanitize):
    """tests/jpeg_enc_rules.cpp: every case and the images of the chunk-boundary call as coefficient records, between two pixel records
    of the format as it was; every stream is the restatement's byte for byte, and the sanitized build ends without a report"""
    pixel = [n for n in TE.NAMES if n.startswith("17x23_4")][:2]
    before = [(n, TE.FIX[n]["pixels"], TE.FIX[n]["mode"], TE.FIX[n]["quality"], TE.FIX[n]["restart"], "RGB") for n in pixel]
    boundary = K.boundary_call()[0]
    ff = dict(w=50, h=33, mode="444", quality=100, restart=0)
    records = [((a.shape[1], a.shape[0], 3, 1, q, int(mode), r), a.tobytes()) for _, a, mode, q, r, _ in before[:1]]
    records += [_record(K.coef(n), K.CASES[n]) for n in NAMES] + [_record(a, ff) for a in boundary]
    records += [((a.shape[1], a.shape[0], 3, 1, q, int(mode), r), a.tobytes()) for _, a, mode, q, r, _ in before[1:]]
    res = TE.run_records(TE._build(tmp_path, sanitize), tmp_path, records)
    assert res[0][0] == TE.FIX[pixel[0]]["jpg"] and res[-1][0] == TE.FIX[pixel[1]]["jpg"]
    for name, (data, coef) in zip(NAMES, res[1:]):
        assert data == K.encoded(name)[0], name
        assert np.array_equal(coef, K.flat(K.coef(name))), name
    for a, (data, _) in zip(boundary, res[1 + len(NAMES):]):
        assert data == E.encode_coef(a, 50, 33, "444", 100, 0)[0]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_decoder_rules_on_the_new_streams(tmp_path, sanitize):
    """tests/jpeg_rules.cpp: coefficients, planes and pixels of every stream are exactly the restatement's, max included, where the
    restatement alone defines the pixels; where a golden exists they are Pillow's"""
    res = TD._run(TD._build(tmp_path, sanitize), tmp_path, [K.encoded(n)[0] for n in NAMES])
    for name, got in zip(NAMES, res):
        _, coef, planes, px = K.decoded(name)
        assert got[0] == 0, name
        assert np.array_equal(got[4], np.concatenate([c.reshape(-1) for c in coef])), name
        assert np.array_equal(got[5], np.concatenate([p.reshape(-1) for p in planes])), name
        assert np.array_equal(got[3], px), name
        if name in FIX:
            assert np.array_equal(got[3], FIX[name][1]), name


# ------------------------------------------------------------------ the entry ----
def test_the_range_checks_of_the_entry_without_a_device():
    """E1 and the ranges E7 has codes for are reported before a device is needed; the index is in the message"""
    from multiviewstitch_amd import _lib as L, processor as P
    lib = L.lib()
    assert hasattr(lib, "mvs_test_jpeg_encode_coef") and "mvs_test_jpeg_encode_coef" in L.EXPORTS
    name = "rand_17x23_420"
    c, good = K.CASES[name], K.flat(K.coef(name))
    n_coef = len(good)
    assert n_coef == 64 * (4 * 4 + 2 * 2 * 2)                        # 2 x 2 MCUs: a luma plane of [4][4] blocks, 3 x 3 of them real
    off, out = np.zeros(3, np.int64), np.zeros(64, np.uint8)
    prm = P.jpeg_encode_params(quality=100, sampling=420, restart_interval=0)

    def call(coef, n=2, w=c["w"], h=c["h"], flags=0, p=prm, capacity=64):
        return lib.mvs_test_jpeg_encode_coef(n, w, h, L.ptr(coef) if coef is not None else None, flags, C.byref(p), L.ptr(off), L.ptr(out), capacity)

    two = np.concatenate([good, good])
    no_device = L.device_count() == 0
    real_luma = 64 * (4 * 1 + 2)                                     # block (2, 1) of the luma plane
    for at, value, ok in ((real_luma, 1024, False), (real_luma, -1025, False), (real_luma, -1024, True), (real_luma, 1023, True),
                          (real_luma + 63, 1024, False), (real_luma + 63, -1024, False), (real_luma + 1, -1023, True),
                          (n_coef + 64 * 16 + 5, 2047, False), (n_coef - 1, -32768, False)):
        bad = two.copy()
        bad[at] = value
        if ok:
            if no_device:                                            # in range: the call gets as far as asking for a device
                assert call(bad) == E_NO_DEVICE, (at, value)
            continue
        assert call(bad) == E_INVALID, (at, value)
        text = lib.mvs_last_error().decode()
        assert f"coef[{at}] = {value}" in text and f"image {at // n_coef}" in text, text
    assert (two[64 * 12:64 * 16] == K.DUMMY).all() and (two[64 * 3:64 * 4] == K.DUMMY).all()   # the dummy row and column hold 32767 and pass
    assert call(None) == E_INVALID
    for kw in (dict(quality=0), dict(sampling=411), dict(restart_interval=-1)):
        assert call(two, p=P.jpeg_encode_params(**{**dict(quality=100, sampling=420, restart_interval=0), **kw})) == E_INVALID, kw
    for kw in (dict(n=0), dict(w=0), dict(h=65536), dict(flags=4), dict(capacity=-1)):
        assert call(two, **kw) == E_INVALID, kw
    if L.device_count() == 0:
        assert call(two) == E_NO_DEVICE
