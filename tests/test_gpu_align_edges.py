"""csrc/align.hip against the oracle on inputs that take every side of its data-dependent branches (tests/align_cases.py; that the
inputs do so is tests/test_align_cases.py's business): posed scenes stage by stage and whole, label-set repairs, ties at a limb's far
end at every level of k_range's first-index rule, and mvs_pca against the exact PCA on small, degenerate and far-away selections.
The bars of the parity checks are those of tests/test_align.py; the PCA's are GPU_FACTOR times the oracle's own recorded worst."""
import numpy as np
import pytest

from tests import align_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def al():
    from multiviewstitch_amd import _lib, alignment
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return alignment


def close(g, o, tol_R=1e-9, tol_t=1e-9, tol_s=1e-11):
    return np.abs(g[0] - o[0]).max() < tol_R and np.abs(g[1] - o[1]).max() < tol_t and abs(g[2] - o[2]) < tol_s


@pytest.mark.parametrize("key", A.FAMILY, ids=lambda k: f"{k[0]} ground{k[1]:+d} view{k[2]:+d}")
def test_gpu_stages_and_align_match_oracle_on_posed_scenes(al, oracle, key):
    """RemoveGround (both values of `which`), InitAlignment (both sides of the ground and view flips) and LocalAlignmentCore (axis
    flip, label-set repair <, =, >, end swaps) on every member of the family, each stage fed with the oracle's output of the one
    before, then Alignment::Align whole and on device arrays."""
    import torch
    sc, w = A.posed(*key), A.family_witness(key, oracle)
    st = w["stage"]
    Al = al.Alignment()
    ggr, gp, gn, gf = Al.RemoveGround(sc["tgt"], sc["t_nrm"], sc["t_faces"], A.DIST)
    assert np.array_equal(gp, st["p"]) and np.array_equal(gn, st["n"]) and np.array_equal(gf, st["f"]) and len(gp) == sc["n_body"]
    assert np.abs(ggr - st["ground_ray"]).max() < 1e-9
    g = Al.InitAlignment(sc["src"], st["p"], st["ground_ray"], sc["view_ray"])
    assert close(g, (st["R"], st["t"], st["scale"]), tol_s=1e-12), (key, g, st["R"], st["t"], st["scale"])
    for (name, edit), l in w["limbs"].items():
        mask, label = A.GROUPS[name]
        sl, tl = A.label_edit(sc["s_labels"], st["t_labels"], edit)
        g = Al.LocalAlignmentCore(st["moved"], sl, st["p"], tl, mask, label)
        assert close(g, (l["R"], l["t"], l["scale"])), (key, name, edit, g, l["R"], l["t"], l["scale"])
    g = Al.Align(sc["src"], sc["s_nrm"], sc["s_labels"], sc["tgt"], sc["t_nrm"], sc["t_faces"], sc["view_ray"], A.DIST)
    o = oracle.align(sc["src"], sc["s_nrm"], sc["s_labels"], sc["tgt"], sc["t_nrm"], sc["t_faces"], sc["view_ray"], A.DIST)
    assert np.isfinite(o["src"]).all()
    assert np.array_equal(g["tgt"], o["tgt"]) and np.array_equal(g["t_normals"], o["t_normals"])
    assert np.array_equal(g["t_facets"], o["t_facets"]) and np.array_equal(g["t_labels"], o["t_labels"])
    assert np.abs(g["ground_ray"] - o["ground_ray"]).max() < 1e-9
    assert np.abs(g["src"] - o["src"]).max() < 1e-8 and np.abs(g["s_normals"] - o["s_normals"]).max() < 1e-8
    dev = torch.device("cuda", 0)
    t, tn = torch.from_numpy(sc["tgt"]).to(dev), torch.from_numpy(sc["t_nrm"]).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(sc["t_faces"], np.int32)).to(dev)
    tl = torch.full((len(sc["tgt"]),), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    d = Al.AlignDev(sc["src"], sc["s_nrm"], sc["s_labels"], t.data_ptr(), tn.data_ptr(), len(sc["tgt"]), tf.data_ptr(), len(sc["t_faces"]), tl.data_ptr(),
                    sc["view_ray"], A.DIST)
    n, f = d["n_t"], d["n_f"]
    assert n == len(g["tgt"]) and f == len(g["t_facets"]) and n < len(sc["tgt"])
    assert np.array_equal(t[:n].cpu().numpy(), g["tgt"]) and np.array_equal(tn[:n].cpu().numpy(), g["t_normals"])
    assert np.array_equal(tf[:f].cpu().numpy(), g["t_facets"]) and np.array_equal(tl[:n].cpu().numpy(), g["t_labels"])
    assert np.array_equal(d["src"], g["src"]) and np.array_equal(d["s_normals"], g["s_normals"]) and np.array_equal(d["ground_ray"], g["ground_ray"])


def test_gpu_far_end_ties_go_to_the_first_index(al, oracle):
    """two coincident far-end points, exactly one of them labelled `label`: which one k_range reports decides a swap that moves
    scale and t by > 1e-2 (tests/test_align_cases.py).  One lane, one wave, one block, one grid-stride trip and one trip less
    one block apart, the copy after and before the original, on the template and on the scan."""
    Al = al.Alignment()
    bad = []
    for name, s, sl, t, tl, mask, label, _, _ in A.tie_family(A.posed(*A.FAMILY[0]), oracle):
        g, o = Al.LocalAlignmentCore(s, sl, t, tl, mask, label), oracle.local_alignment_core(s, sl, t, tl, mask, label)
        if not close(g, o):
            bad.append((name, g[2], o[2]))
    assert not bad, bad


def test_gpu_label_31(al, oracle):
    """bit 31 of a mask and of the set of labels present (which leaves the device in a double)"""
    Al = al.Alignment()
    case = A.posed(*A.FAMILY[0])
    for edit in (None, ("ARM_L", "tmpl", 2, 3), ("ARM_L", "scan", 3, 2)):
        args = A.label31_arrays(case, oracle, edit)
        assert close(Al.LocalAlignmentCore(*args), oracle.local_alignment_core(*args)), edit
    p, lab, mask = A.pca_cases()["label 31 only"]
    g, o = al.pca(p, lab, mask), oracle.pca(p, lab, mask)
    assert np.array_equal(g[1], o[1]) and np.abs(g[0] - o[0]).max() < 1e-13 and np.abs(g[3] - o[3]).max() < 1e-11


def test_gpu_pca_is_within_ten_times_the_oracles_worst_of_the_exact_pca(al):
    worst = dict(bary=(0.0, ""), eval=(0.0, ""), orth=(0.0, ""), axis_k=(0.0, ""))
    bound = A.pca_bounds(A.GPU_FACTOR)
    bad = []
    for name, (p, lab, mask) in A.pca_cases().items():
        e = A.pca_errors(al.pca(p, lab, mask), A.pca_reference_of(name))
        if not (e["bbox"] and e["sign"] and all(e[k] <= bound[k] for k in worst)):
            bad.append((name, e))
        for k in worst:
            if e[k] > worst[k][0]:
                worst[k] = (e[k], name)
    print("mvs_pca against the exact PCA, worst over pca_cases():", {k: f"{v:.3g} ({n})" for k, (v, n) in worst.items()})
    assert not bad, (bad, bound)


def test_gpu_pca_of_coincident_points(al):
    for name, (p, dyadic) in A.coincident_cases().items():
        b, bb, ax, ev = al.pca(p)
        assert np.isfinite(ax).all() and np.abs(ax @ ax.T - np.eye(3)).max() <= A.GPU_FACTOR * A.ORACLE_WORST_ORTH, name
        assert all(a[np.argmax(np.abs(a))] > 0 for a in ax) and np.array_equal(bb, np.stack([p[0], p[0]])), name
        if dyadic:
            assert np.array_equal(b, p[0]) and np.array_equal(ev, np.zeros(3)), (name, b, ev)
        else:
            assert np.abs(b - p[0]).max() <= len(p) * A.EPS * np.abs(p).max() and np.abs(ev).max() <= A.coincident_eval_bound(p), (name, ev)


def test_gpu_selections_of_0_and_1_points_are_degenerate_and_write_nothing(al, oracle):
    from multiviewstitch_amd import _lib
    for name, (p, n, lab, mask) in A.degenerate_selections().items():
        rc, out = A.raw_pca(_lib.lib().mvs_pca, p, n, lab, mask)
        assert rc == A.raw_pca(oracle.lib().orc_pca, p, n, lab, mask)[0] == A.DEGENERATE, (name, rc)
        assert all((o == A.SENTINEL).all() for o in out), name
    for V in (0, 1):
        pts, faces = np.arange(3.0 * V).reshape(V, 3) + 0.5, np.zeros((V, 3), np.int32)
        rc, nv, nf, p, nr, f, gr = A.raw_remove_ground(_lib.lib().mvs_remove_ground, pts, faces)
        assert rc == A.raw_remove_ground(oracle.lib().orc_remove_ground, pts, faces)[0] == A.DEGENERATE, (V, rc)
        assert (nv, nf) == (V, V) and np.array_equal(p, pts) and np.array_equal(nr, pts[::-1] + 1.0) and np.array_equal(f, faces) and (gr == A.SENTINEL).all()
    p, n, lab, mask = A.degenerate_selections()["mask matches one"]                       # the entry still works after the refusals
    lab = lab.copy()
    lab[7] = 20
    assert np.array_equal(al.pca(p, lab, mask)[1], np.stack([p[[7, 123]].min(0), p[[7, 123]].max(0)]))
