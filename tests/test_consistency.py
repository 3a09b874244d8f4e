"""Depth-consistency filter (SURVEY §8(f) row 2, R/Processor/Processor.cpp:29-126): oracle properties on CPU, bit-exact
parity of the HIP kernel against the oracle on the GPU, on rendered scenes.  Raster edges, non-finite depths and the double -> int
rule: tests/test_consist_host.py and tests/test_gpu_consist.py."""
import numpy as np
import pytest

from multiviewstitch_amd import scene as S

MN, MX = S.MIN_DSP, S.MAX_DSP


@pytest.fixture(scope="module")
def seq():
    cams, d = S.make_sequence(5, 160, 120, 3.0)
    rng = np.random.default_rng(4)
    noisy = d.copy()
    m = rng.random(d.shape) < 0.03                      # gross depth errors the filter is there to remove
    noisy[m] *= rng.uniform(0.6, 1.5, m.sum()).astype(np.float32)
    noisy[:, :3, :] = 0.5                               # out-of-range inverse depths
    return cams, d, noisy


def test_oracle_keeps_consistent_surface_and_removes_outliers(oracle, seq):
    cams, d, noisy = seq
    clean = oracle.check_consistency_seq(d, cams, MN, MX, 4)
    assert np.all((clean == d) | (clean == 0))
    fg = d > 0
    assert (clean[fg] == d[fg]).mean() > 0.9             # a rendered surface is self-consistent (occlusion rims go)
    out = oracle.check_consistency_seq(noisy, cams, MN, MX, 4)
    assert np.all((out == noisy) | (out == 0)) and not out[:, :3, :].any()
    bad = (noisy != d) & fg
    good = (noisy == d) & fg
    # the test is a reprojection round trip, not a depth comparison: with a 3 degree baseline at this resolution it
    # catches a third of the gross errors — far more than it removes of the untouched surface
    assert (out[bad] == 0).mean() > 0.25 and (out[bad] == 0).mean() > 3 * (out[good] == 0).mean()
    # the sequence driver = the core applied frame by frame against the ORIGINAL neighbours, previous first
    for i in (0, 2, 4):
        refs = [j for j in (i - 1, i + 1) if 0 <= j < 5]
        one = oracle.check_consistency(noisy[i], cams[i], [noisy[j] for j in refs], [cams[j] for j in refs], MN, MX, 4)
        assert np.array_equal(one, out[i])
    # a tighter threshold never keeps more
    tight = oracle.check_consistency_seq(noisy, cams, MN, MX, 0)
    assert np.all((tight == out) | (tight == 0)) and (tight != 0).sum() < (out != 0).sum()


@pytest.mark.gpu
def test_gpu_consistency_is_bit_exact(oracle, seq):
    from multiviewstitch_amd import processor
    cams, d, noisy = seq
    for thr in (0, 1, 4):
        assert np.array_equal(processor.CheckConsistency(cams, noisy, MN, MX, thr), oracle.check_consistency_seq(noisy, cams, MN, MX, thr))
    got = processor.CheckConsistencyCore(cams[2], [cams[1], cams[3]], noisy[2], [noisy[1], noisy[3]], MN, MX, 4)
    assert np.array_equal(got, oracle.check_consistency(noisy[2], cams[2], [noisy[1], noisy[3]], [cams[1], cams[3]], MN, MX, 4))
    got = processor.CheckConsistencyCore(cams[2], [], noisy[2], [], MN, MX, 4)          # no references: range test only
    assert np.array_equal(got, np.where((noisy[2] >= np.float32(MN)) & (noisy[2] <= MX), noisy[2], 0))


@pytest.mark.gpu
def test_gpu_consistency_full_size_device_path(oracle):
    """1280x960 x 6 frames resident in HBM: parity with the oracle on two frames, idempotence-style properties on all."""
    import torch
    from multiviewstitch_amd import processor
    dev = torch.device("cuda", 0)
    cams, d = S.make_sequence(6, 1280, 960, 2.0, device=dev)
    din = torch.from_numpy(d).to(dev)
    dout = torch.empty_like(din)
    processor.CheckConsistency(cams, din.data_ptr(), MN, MX, 4, out_dev=dout.data_ptr())
    out = dout.cpu().numpy()
    assert np.all((out == d) | (out == 0)) and (out[d > 0] != 0).mean() > 0.9
    for i in (0, 3):
        refs = [j for j in (i - 1, i + 1) if 0 <= j < 6]
        assert np.array_equal(out[i], oracle.check_consistency(d[i], cams[i], [d[j] for j in refs], [cams[j] for j in refs], MN, MX, 4))
