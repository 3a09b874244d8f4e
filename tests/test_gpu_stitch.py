"""The stitch tail of Processor::AlignmentSeq on the GPU (R/Processor/Processor.cpp:952-1105): the visibility cull in both
modes, the PSR files, the Poisson-model trim and the PlyObj vertex normals of a general mesh, against the numpy checker
(tests/ref_stitch.py) built from oracle primitives.  Masks, counts, normals and files are bit / byte identical."""
import functools

import numpy as np
import pytest

from multiviewstitch_amd import _lib
from multiviewstitch_amd import io as mio
from multiviewstitch_amd import scene as S
from oracle import binding as O
from tests import ref_stitch as RS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def srt():
    from multiviewstitch_amd import srt
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return srt


def same_bits(a, b):
    """bit-equal doubles, NaN in the same places (the NaN payloads of the two processors may differ)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


@functools.lru_cache(maxsize=1)
def four_sequences():
    """4 sequences of 3-8 cameras (one at 64x48, the others 80x60), random SRTs with s in [0.8, 1.25]; the points of sequence k
    are the depth_to_model outputs of two views of the synthetic scene in k's frame, plus edge points of k's cameras."""
    sc = S.make_scene(0, n_views=8)
    scales, Rs, ts, cams = S.make_stitch_sequences([3, 5, 8, 4], [(80, 60), (80, 60), (64, 48), (80, 60)], [2.4, 2.4, 2.4, 2.4])
    rng = np.random.default_rng(5)
    pts, nrm = [], []
    for k in range(4):
        wp, wn = [], []
        for v in (2 * k, 2 * k + 1):
            p, n, _, _ = O.depth_to_model(sc.depth[v], sc.cams[v], S.MIN_DSP, S.MAX_DSP, S.SMOOTH)
            a, b = O.srt_apply(p, n, *sc.srt[v])
            wp.append(a); wn.append(b)
        lp, ln = O.srt_apply(np.concatenate(wp), np.concatenate(wn), scales[k], Rs[k], ts[k], inverse=True)
        edge = np.concatenate([RS.edge_points(c, rng, n=4) for c in cams[k]])
        pts.append(np.concatenate([lp, edge]))
        nrm.append(np.concatenate([ln, np.tile([0.0, 0.0, 1.0], (len(edge), 1))]))
    return scales, Rs, ts, cams, pts, nrm


def test_cull_parity_both_modes(srt):
    scales, Rs, ts, cams, pts, _ = four_sequences()
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    keep, nk = srt.visibility_cull(np.concatenate(pts), scales, Rs, ts, cams, mode=_lib.CULL_SEQUENCES, seg_off=off)
    ref = RS.cull_sequences(pts, scales, Rs, ts, cams)
    for k in range(4):
        assert np.array_equal(keep[off[k]:off[k + 1]].astype(bool), ref[k]), k
        assert nk[k] == ref[k].sum()
        assert 0.10 <= 1 - ref[k].mean() <= 0.60, (k, 1 - ref[k].mean())       # every sequence culls 10-60 %
    # AllSeqProj: the world points (each sequence mapped forward) as one segment, and as two
    world = np.concatenate([O.srt_apply(pts[k], None, scales[k], Rs[k], ts[k])[0] for k in range(4)])
    ref = RS.cull_all_seq(world, scales, Rs, ts, cams)
    assert 0.05 < 1 - ref.mean() < 0.95
    for seg in ([0, len(world)], [0, 1000, len(world)]):
        keep, nk = srt.visibility_cull(world, scales, Rs, ts, cams, mode=_lib.CULL_ALL_SEQ, seg_off=seg)
        assert np.array_equal(keep.astype(bool), ref)
        assert list(nk) == [int(ref[a:b].sum()) for a, b in zip(seg[:-1], seg[1:])]


def test_cull_dev_form(srt):
    torch = pytest.importorskip("torch")
    scales, Rs, ts, cams, pts, _ = four_sequences()
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    allp = np.concatenate(pts)
    dp = torch.from_numpy(allp).to("cuda")
    dk = torch.empty(len(allp), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nk = srt.visibility_cull_dev(dp.data_ptr(), off, scales, Rs, ts, cams, dk.data_ptr(), mode=_lib.CULL_SEQUENCES)
    keep, nk_host = srt.visibility_cull(allp, scales, Rs, ts, cams, mode=_lib.CULL_SEQUENCES, seg_off=off)
    assert np.array_equal(dk.cpu().numpy(), keep) and np.array_equal(nk, nk_host)


def test_cull_scan_scale(srt):
    """8 sequences x 16 cameras, ~2 M points on the surface of the synthetic body's bounding shell."""
    n_seq, per = 8, 250_000
    scales, Rs, ts, cams = S.make_stitch_sequences([16] * n_seq, [(1280, 960)] * n_seq, [2.2] * n_seq, seed=21)
    rng = np.random.default_rng(9)
    pts = []
    for k in range(n_seq):
        d = rng.normal(size=(per, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        w = d * rng.uniform(0.85, 1.15, (per, 1))
        pts.append(O.srt_apply(np.ascontiguousarray(w), None, scales[k], Rs[k], ts[k], inverse=True)[0])
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    keep, nk = srt.visibility_cull(np.concatenate(pts), scales, Rs, ts, cams, mode=_lib.CULL_SEQUENCES, seg_off=off)
    ref = RS.cull_sequences(pts, scales, Rs, ts, cams)
    for k in range(n_seq):
        assert np.array_equal(keep[off[k]:off[k + 1]].astype(bool), ref[k]), k
        assert nk[k] == ref[k].sum()
    assert 0.10 <= 1 - keep.mean() <= 0.60


@pytest.mark.parametrize("truncate", [False, True])
def test_psr_files_byte_identical(srt, tmp_path, truncate):
    from multiviewstitch_amd import processor
    scales, Rs, ts, cams, pts, nrm = four_sequences()
    paths = []
    for k in range(4):
        paths.append(str(tmp_path / f"seq{k}.npts"))
        mio.write_npts(paths[-1], np.clip(np.nan_to_num(pts[k], nan=0.0), -1e30, 1e30), nrm[k])      # (text a float32 reads back)
    res = tmp_path / "Result"
    res.mkdir()
    nk = processor.StitchPointSets(paths, scales, Rs, ts, cams, str(res), truncate=truncate)
    names = [f"PSR{k}.obj" for k in range(4)] + ["PSR.npts"]
    got = {name: (res / name).read_bytes() for name in names}
    rp, rn = zip(*[mio.read_npts(p) for p in paths])                 # what the entry read: float32 text -> double
    out, nk_ref = RS.stitch(list(rp), list(rn), scales, Rs, ts, cams, truncate=truncate)
    assert np.array_equal(nk, nk_ref)
    for k, (wp, wn) in enumerate(out):                                # (same paths: WriteObj prints the file name in its header)
        assert len(wp) == (nk_ref[k] if truncate else len(rp[k]))
        mio.WriteObj(str(res / f"PSR{k}.obj"), wp, wn)
    mio.write_npts(str(res / "PSR.npts"), np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]))
    for name in names:
        assert got[name] == (res / name).read_bytes(), name


def model_mesh():
    """a closed body of the scene's size and a small closed component inside it (RetainConnectRegion drops it)"""
    d, f = S.geodesic_sphere(14)
    rng = np.random.default_rng(4)
    body = d * (1.0 + 0.1 * np.sin(3 * d[:, :1]) * np.cos(2 * d[:, 1:2]))
    d2, f2 = S.geodesic_sphere(3)
    small = 0.1 * d2 + np.array([0.2, -0.1, 0.3])
    pts = np.concatenate([body, small]) + rng.normal(scale=1e-4, size=(len(body) + len(small), 3))
    faces = np.concatenate([f, f2 + len(body)]).astype(np.int32)
    return pts, faces


@pytest.mark.parametrize("with_vn", [True, False])
@pytest.mark.parametrize("all_seq_proj", [True, False])
def test_model_cull_byte_identical(srt, tmp_path, with_vn, all_seq_proj):
    from multiviewstitch_amd import processor
    scales, Rs, ts, cams, _, _ = four_sequences()
    pts, faces = model_mesh()
    model = str(tmp_path / "Model.obj")
    mio.WriteObj(model, pts, O.vertex_normals(pts, faces, kind="plyobj") if with_vn else None, faces)
    out = str(tmp_path / "Model_cut.obj")
    V, F = processor.CullPoissonModel(model, scales, Rs, ts, cams, out, all_seq_proj=all_seq_proj)
    with open(out, "rb") as fh:
        got = fh.read()
    rp, rn, rf = mio.ReadObj(model)                                  # what ReadObj holds (float32 text -> double)
    assert (len(rn) == len(rp)) == with_vn
    ep, en, ef = RS.cull_model(rp, rn if with_vn else None, rf, scales, Rs, ts, cams, all_seq_proj=all_seq_proj)
    assert (V, F) == (len(ep), len(ef))
    assert len(ep) < len(rp) and len(ef) > 0
    mio.WriteObj(out, ep, en, ef)                                    # (same path: WriteObj prints the file name in its header)
    with open(out, "rb") as fh:
        assert got == fh.read()


def test_vertex_normals_general_meshes(srt):
    rng = np.random.default_rng(8)
    cases = []
    for V, F in ((50, 80), (1000, 3000), (5000, 4000)):             # random triangle soups (unused vertices included)
        cases.append((rng.normal(size=(V, 3)), rng.integers(0, V, size=(F, 3)).astype(np.int32)))
    p = rng.normal(size=(12, 3))
    p[1] = p[0] + 3e-7                                                # an edge shorter than 1e-6: the 1e9 rescue
    p[5] = np.array([0.0, 0.0, 0.0]); p[6] = np.array([1.0, 0.0, 0.0]); p[7] = np.array([2.0, 0.0, 0.0])   # zero area
    f = np.array([[0, 1, 2], [1, 3, 2], [5, 6, 7], [5, 6, 8], [2, 2, 3], [3, 4, 9], [9, 4, 3]], np.int32)   # vertex 10, 11 isolated
    cases.append((p, f))
    hub = 1500                                                         # a hub vertex with 1500 facets (a fan)
    ang = np.linspace(0, 2 * np.pi, hub + 1)
    fan = np.concatenate([[[0, 0, 0]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(5 * ang)], 1)])
    ff = np.stack([np.zeros(hub), 1 + np.arange(hub), 2 + np.arange(hub)], 1).astype(np.int32)
    cases.append((fan, ff[rng.permutation(hub)]))
    n = 1415                                                           # ~2 M-vertex scan mesh: a height field
    x, y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    grid = np.stack([x.ravel(), y.ravel(), 0.1 * np.sin(4 * x.ravel()) * np.cos(3 * y.ravel())], 1)
    i = np.arange(n - 1)
    a = (i[:, None] * n + i[None, :]).ravel()
    quads = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)]).astype(np.int32)
    cases.append((grid, quads))
    for k, (pts, faces) in enumerate(cases):
        got = srt.mesh_vertex_normals(pts, faces)
        ref = O.vertex_normals(pts, faces, kind="plyobj")
        assert same_bits(got, ref), k
    p, f = cases[3]
    got = srt.mesh_vertex_normals(p, f)
    assert np.isnan(got[[7, 10, 11]]).all() and not np.isnan(got[[0, 1]]).any()


def test_vertex_normals_reject_an_index_out_of_range(srt):
    with pytest.raises(_lib.MvsError) as e:
        srt.mesh_vertex_normals(np.zeros((3, 3)), np.array([[0, 1, 3]], np.int32))
    assert e.value.code == -2
