"""Host side of the depth-consistency tests: the numpy restatement (tests/ref_consist.py) equals the oracle bit for bit on every
scene of tests/consist_scenes.py, and those scenes reach what they were built for — every branch of the filter, every edge of the
double -> int rule, pixels exactly on the threshold, every reference slot, every poison value where a live pixel reads it.  The GPU
tests (tests/test_gpu_consist.py) compare the kernels with the same expected values."""
import numpy as np
import pytest

from tests import consist_scenes as CS
from tests import ref_consist as RC


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """equal as uint32, which tells -0.0 from 0.0 and one NaN from another"""
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("ref_list", CS.REF_LISTS)
def test_restatement_equals_the_oracle_on_the_edge_scene(oracle, ref_list):
    cur, d, rcams, rds = CS.edge_case(ref_list)
    for thr in CS.THRESHOLDS:
        want = oracle.check_consistency(d, cur, rds, rcams, CS.MN, CS.MX, thr)
        e = CS.expected_edge(ref_list, thr)
        assert same_bits(e.out, want), (ref_list, thr)
        assert np.array_equal(e.out != 0, e.reason == RC.KEPT) and np.array_equal(e.ref >= 0, (e.reason != RC.KEPT) & (e.reason != RC.OWN_RANGE))


@pytest.mark.parametrize("size", CS.SIZES)
def test_restatement_equals_the_oracle_on_degenerate_rasters(oracle, size):
    cur, d, rcams, rds = CS.size_scene(*size)
    assert d.shape == (size[1], size[0])
    for thr in CS.THRESHOLDS:
        want = oracle.check_consistency(d, cur, list(rds), list(rcams), CS.MN, CS.MX, thr)
        assert same_bits(CS.expected_size(*size, thr).out, want), (size, thr)


@pytest.mark.parametrize("n", CS.SEQ_FRAMES)
def test_restatement_equals_the_oracle_on_sequences(oracle, n):
    cams, d = CS.sequence(n)
    assert d.shape == (n, CS.H, CS.W) and d[0].size % 256 != 0
    for thr in CS.THRESHOLDS:
        out, res = CS.expected_seq(n, thr)
        assert same_bits(out, oracle.check_consistency_seq(d, cams, CS.MN, CS.MX, thr)), (n, thr)
        for i, r in enumerate(res):                                   # the driver = the core, previous frame first
            nb = RC.neighbours(i, n)
            assert same_bits(r.out, oracle.check_consistency(d[i], cams[i], [d[k] for k in nb], [cams[k] for k in nb], CS.MN, CS.MX, thr))


def test_edge_scene_reaches_every_class():
    runs = {(rl, thr): CS.expected_edge(rl, thr) for rl in CS.REF_LISTS for thr in CS.THRESHOLDS}
    reasons = sum(np.bincount(e.reason.ravel(), minlength=6) for e in runs.values())
    print("pixels per reason over all runs:", dict(zip(RC.REASONS, reasons.tolist())))
    assert (reasons > 0).all(), dict(zip(RC.REASONS, reasons.tolist()))
    for name in RC.COUNTS[:-1]:                                       # the edges of the double -> int rule
        total = sum(e.counts[name] for e in runs.values())
        print(name, total)
        assert total > 0, name
    for thr in (0, 1, 2):                                             # `>` against `>=`
        on = sum(e.counts["on_threshold"] for (rl, t), e in runs.items() if t == thr)
        print("on the threshold", thr, on)
        assert on > 0, thr
    slots = sum(np.bincount(e.ref.ravel() + 1, minlength=5)[1:] for (rl, t), e in runs.items() if len(rl) == 4)
    print("pixels decided per reference slot, four-reference runs:", slots.tolist())
    assert (slots > 0).all(), slots
    assert CS.W * CS.H % 256 != 0 and CS.W * CS.H > 4 * 256


@pytest.mark.parametrize("wrong", [RC.cvt_floor, RC.cvt_bare])
def test_a_wrong_conversion_rule_would_show(wrong):
    """floor instead of truncation, or a bare (int) that turns NaN into 0: the edge scene gives another raster under either"""
    differ = 0
    for rl in CS.REF_LISTS:
        cur, d, rcams, rds = CS.edge_case(rl)
        for thr in CS.THRESHOLDS:
            got = RC.check_core(d, cur, rds, rcams, CS.MN, CS.MX, thr, cvt=wrong).out
            differ += int((bits(got) != bits(CS.expected_edge(rl, thr).out)).sum())
    print(wrong.__name__, "pixels that differ over all runs:", differ)
    assert differ > 0


def test_every_poison_value_is_read_by_a_live_pixel():
    p = CS.poison()
    assert np.isnan(p[0]) and np.isposinf(p[1]) and np.isneginf(p[2]) and p[3] < 0 and np.signbit(p[4]) and p[4] == 0 and p[5] == 0
    assert 0 < p[6] < np.finfo(np.float32).tiny
    assert p[7] < p[8] < p[9] and p[10] < p[11] < p[12]                # float32(min_dsp), float32(max_dsp) and their neighbours
    assert float(p[7]) < CS.MN < float(p[9]) and float(p[10]) < CS.MX < float(p[12])
    # the edge scene: row CUR_POISON of the current raster; row REF_POISON of reference 0, where live pixels of the plane land
    cur, d, rcams, rds = CS.edge_case((0,))
    row, col = CS.CUR_POISON
    assert same_bits(d[row, col:col + len(p)], p)
    row, col = CS.REF_POISON
    assert same_bits(rds[0][row, col:col + len(p)], p)
    read = set(CS.expected_edge((0,), 5).read[0].tolist())
    assert all(row * CS.W + c in read for c in range(col, col + len(p)))
    # the sequences: a poisoned frame is the current one in its own turn and the reference in its neighbours'
    cams, d = CS.sequence(5)
    _, res = CS.expected_seq(5, 5)
    for f, row in CS.SEQ_POISON:
        assert same_bits(d[f, row, CS.SEQ_COL:CS.SEQ_COL + len(p)], p)
        read = set()
        for i in RC.neighbours(f, 5):
            read |= set(res[i].read[RC.neighbours(i, 5).index(f)].tolist())
        assert all(row * CS.W + c in read for c in range(CS.SEQ_COL, CS.SEQ_COL + len(p))), (f, row)
    # the degenerate rasters hold as much of the list as half the raster takes
    for w, h in CS.SIZES:
        cur, d, rcams, rds = CS.size_scene(w, h)
        k = min(len(p), w * h // 2)
        assert same_bits(d.ravel()[1:1 + k], p[:k]) and same_bits(rds[0].ravel()[1:1 + k], p[:k])
        if k:
            e = CS.expected_size(w, h, 5)
            assert (e.reason == RC.OWN_RANGE).sum() >= min(k, 11)     # 11 of the 13 values are out of range
