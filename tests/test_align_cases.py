"""Conditions on the INPUTS of tests/test_gpu_align_edges.py, checked on the CPU oracle alone (tests/align_cases.py): the posed
family takes every side of every branch of csrc/align.hip and stays clear of every knife-edge; the tie inputs really are decided by
the first-index rule; the oracle's PCA is within ORACLE_WORST_* of the exact restatement on small, degenerate and far-away clouds."""
import numpy as np

from tests import align_cases as A
from tests.util import body_scene


def test_posed_default_is_body_scene():
    a, b = A.posed(), body_scene(5, 8, 12)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    h = A.posed("half_x")                                             # a rigid motion of the same scan
    d = lambda s: np.linalg.norm(s["tgt"][:50, None] - s["tgt"][None, :50], axis=2)          # noqa: E731
    assert np.abs(d(a) - d(h)).max() < 1e-12 and not np.allclose(a["tgt"], h["tgt"])


def test_family_takes_every_side_of_every_branch(oracle):
    """the coverage condition: over FAMILY x (no edit + EDITS) every witness takes every value at least once — and every decision
    has a margin that the device's other summation order cannot cross; no limb has parallel axes (finite R)."""
    seen = {k: set() for k in ("which", "ground_flip", "view_flip", "flip", "sets", "lab1_eq", "lab2_eq")}
    for key in A.FAMILY:
        w = A.family_witness(key, oracle)
        for k in ("which", "ground_flip", "view_flip"):
            seen[k].add(w[k])
        assert abs(w["ground_dot"]) > A.DOT_MARGIN and abs(w["view_dot"]) > A.DOT_MARGIN, (key, w["ground_dot"], w["view_dot"])
        assert w["ground_flip"] == (w["which"] == 1)                  # (both are the sign of the first pivot: the issue's "behaves the same way")
        assert len(w["limbs"]) == 4 + len(A.EDITS)
        for (name, edit), l in w["limbs"].items():
            tag = (key, name, edit)
            assert l["status"] == 0 and l["finite"], tag
            assert abs(l["flip_dot"]) > A.DOT_MARGIN and l["sin_axes"] > A.SIN_MARGIN and l["margin"] > A.FAR_MARGIN, (tag, l)
            for k in ("flip", "sets", "lab1_eq", "lab2_eq"):
                seen[k].add(l[k])
            if edit is not None:                                      # an edit does what it is for
                assert l["sets"] == (">" if edit[1] == "scan" else "<"), tag
                if edit[2] == A.GROUPS[name][1]:                      # the end label itself went missing: both ends swap
                    assert not l["lab1_eq"] and not l["lab2_eq"], tag
            else:
                assert l["sets"] == "="
    assert seen == dict(which={1, 2}, ground_flip={True, False}, view_flip={True, False}, flip={True, False}, sets={"<", "=", ">"},
                        lab1_eq={True, False}, lab2_eq={True, False}), seen


def test_tie_inputs_are_decided_by_the_first_index(oracle):
    """the far end is a clear extreme (so its exact copy ties with it and with nothing else), the pair sits where TIE_DISTANCES
    says, the oracle reads the label at the FIRST of the two, and exchanging the two labels moves the result by far more than
    the parity tolerances (1e-9 / 1e-11): a wrong tie rule on the device cannot pass."""
    fam = A.tie_family(A.posed(*A.FAMILY[0]), oracle)
    assert len(fam) == 2 * len(A.TIE_DISTANCES) * 2
    for name, s, sl, t, tl, mask, label, sl2, tl2 in fam:
        side = name.split()[0]
        w = A.limb_witness(oracle, s, sl, t, tl, mask, label)
        assert w["status"] == 0 and w["finite"] and w["margin"] > 1e-5 and w["sin_axes"] > A.SIN_MARGIN, (name, w)
        far = w["far_src" if side == "tmpl" else "far_tgt"]["hi"]
        pts, lab, lab2 = (s, sl, sl2) if side == "tmpl" else (t, tl, tl2)
        d = int(name.split()[2])
        i = far["index"]
        assert i % A.TPB == A.TIE_LANE % A.TPB and np.array_equal(pts[i], pts[i + d])      # (the witness's argmax is the first index)
        assert (lab[i] == label) != (lab[i + d] == label) and lab2[i] == lab[i + d] and lab2[i + d] == lab[i]
        assert (mask >> lab[i]) & 1 and (mask >> lab[i + d]) & 1
        assert w["lab1_eq" if side == "tmpl" else "lab2_eq"] == (lab[i] == label)
        R2, t2, s2 = oracle.local_alignment_core(s, sl2, t, tl2, mask, label)
        assert np.array_equal(R2, w["R"])                                                 # (labels do not enter the axes)
        assert abs(s2 - w["scale"]) > 1e-2 and np.abs(t2 - w["t"]).max() > 1e-2, (name, s2, w["scale"])


def test_label_31_is_a_label_like_any_other(oracle):
    case = A.posed(*A.FAMILY[0])
    st = A.stage_inputs(case, oracle)
    for edit in (None, ("ARM_L", "tmpl", 2, 3), ("ARM_L", "scan", 3, 2)):
        sl, tl = A.label_edit(case["s_labels"], st["t_labels"], edit)
        want = oracle.local_alignment_core(st["moved"], sl, st["p"], tl, A.ARM_L, 4)
        got = oracle.local_alignment_core(*A.label31_arrays(case, oracle, edit))
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and np.isfinite(want[0]).all()


def test_oracle_pca_is_within_its_recorded_worst_of_the_exact_pca(oracle):
    worst = dict(bary=(0.0, ""), eval=(0.0, ""), orth=(0.0, ""), axis_k=(0.0, ""))
    compared = 0
    for name, (p, lab, mask) in A.pca_cases().items():
        ref = A.pca_reference_of(name)
        e = A.pca_errors(oracle.pca(p, lab, mask), ref)
        assert e["bbox"] and e["sign"], (name, e)
        compared += sum(g >= A.GAP_MIN for g in ref["gaps"])
        for k in worst:
            if e[k] > worst[k][0]:
                worst[k] = (e[k], name)
    print("oracle.pca against the exact PCA, worst over pca_cases():", {k: f"{v:.3g} ({n})" for k, (v, n) in worst.items()})
    assert compared > 2 * len(A.pca_cases())                          # (most axes ARE compared)
    bound = A.pca_bounds()
    assert all(worst[k][0] <= bound[k] for k in worst), (worst, bound)
    assert all(worst[k][0] >= bound[k] / 4 for k in worst), ("the recorded constants are stale", worst, bound)
    ref = A.pca_reference_of("collinear")
    assert abs(ref["evals"][1]) < 1e-50 * ref["evals"][0] and ref["gaps"][0] == 1.0       # (exactly collinear in doubles)


def test_oracle_pca_of_coincident_points(oracle):
    for name, (p, dyadic) in A.coincident_cases().items():
        b, bb, ax, ev = oracle.pca(p)
        assert np.isfinite(ax).all() and np.abs(ax @ ax.T - np.eye(3)).max() <= A.ORACLE_WORST_ORTH, name
        assert all(a[np.argmax(np.abs(a))] > 0 for a in ax) and np.array_equal(bb, np.stack([p[0], p[0]])), name
        if dyadic:
            assert np.array_equal(b, p[0]) and np.array_equal(ev, np.zeros(3)), (name, b, ev)
        else:
            assert np.abs(b - p[0]).max() <= len(p) * A.EPS * np.abs(p).max() and np.abs(ev).max() <= A.coincident_eval_bound(p), (name, ev)


def test_oracle_degenerate_selections_and_remove_ground_of_nothing(oracle):
    for name, (p, n, lab, mask) in A.degenerate_selections().items():
        rc, out = A.raw_pca(oracle.lib().orc_pca, p, n, lab, mask)
        assert rc == A.DEGENERATE and all((o == A.SENTINEL).all() for o in out), (name, rc)
    for V in (0, 1):
        pts, faces = np.arange(3.0 * V).reshape(V, 3) + 0.5, np.zeros((V, 3), np.int32)
        rc, nv, nf, p, nr, f, gr = A.raw_remove_ground(oracle.lib().orc_remove_ground, pts, faces)
        assert rc == A.DEGENERATE and (nv, nf) == (V, V) and np.array_equal(p, pts) and np.array_equal(f, faces) and (gr == A.SENTINEL).all()
