"""The bytes of the association (csrc/assoc.hip, csrc/assoc_dev.h), recorded: for every case below, pass by pass, the sha256 of the raw
bytes of d2min, top_idx, valid, controls (the other tests hold them to 1e-12 only), the ball counts and the node graph.  The library is
built with -ffp-contract=off and the searches are deterministic (no atomics on the data path), so these digests are a function of the
written operations and their order; tests/test_gpu_assoc_bits.py holds every build to the recording in tests/golden/assoc_bits.json.

Counts: a ball with >= max_result members drops the node and the waves stop counting at a moment that depends on their timing, so only
"full" is defined for it (tests.util.counts_match): column 0 is clamped to max_result and column 1 of such a row is zeroed.

The scenes are tests.util.scene_and_target, the nodes oracle.uniform_sampling(verts, 16), as in tests/test_gpu_deform.py:
  fused/c0, fused/c1   the first pass of a fit (k_assoc_local with heavy_rows = 64 + the heavy-node pass)
  passes/c1, passes/c2 five passes (unbounded, unbounded, bounded: near / mid / heavy), set_vertices back to rest, three more; config 1
                       searches its node graph by brute force, config 2 on the node grid (k_assoc_heavy_knn, bounded graph queries)
  far, one_point, nan, top3_graph3, five_nodes
                       the inputs of test_bounded_passes_on_odd_inputs_match_oracle, five passes each
  full_ball, full_ball/8
                       config 1 with max_result = 64 and 8: full balls on the unbounded and on the bounded path (two unbounded passes —
                       the second association of a fit never searches bounded — and three bounded ones); at 8 the balls of the near
                       class (a handful of members) are full too.  `full_nodes`: how many nodes of the pass had a full ball
  sharded/c1           two handles of one view each (index_base set) through assoc_dmin -> minimum -> assoc_select -> assoc_merge(.., 2)
                       -> solve, three outer iterations, then one owner-merges round (assoc_merge_block + set_node_targets_dev)
  group/c1, group/c2   two handles stepped twice alone, then three passes through mvs_deform_group_iterate (k_assoc_prep_multi /
                       k_assoc_all_multi).  The library declines a group whose node graphs are not searched on the grid (fewer than
                       1024 nodes: config 1) — the handles then step alone and the recording says so (`grouped`); config 2 qualifies
  ties, ties/near      a few hundred exact copies of one target point that heads the list of the node with the largest ball that is
                       not full (found by a run without the copies): more float ties than merge slots in the heavy paths.  `ties` on
                       the `far` target (every ball there is full, the lists are never read), `ties/near` on the target itself.
                       Compared against the recording only.

A deliberate change of the association's arithmetic re-records: build the library, then on a GPU
  python scripts/record_assoc_bits.py --parent $(git rev-parse HEAD) --out tests/golden/assoc_bits.json
`--only <case> ...` records some cases; without --out the JSON goes to stdout."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = ("fused/c0", "fused/c1", "passes/c1", "passes/c2", "far", "one_point", "nan", "top3_graph3", "five_nodes", "full_ball", "full_ball/8",
         "sharded/c1", "group/c1", "group/c2", "ties", "ties/near")
N_COPIES = 300


def digest(a) -> str:
    """sha256 of the raw bytes of an array, in C order (NaNs by their bytes)"""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def clamp_counts(counts, max_result):
    c = np.array(counts, np.int32).reshape(-1, 2)
    full = c[:, 0] >= max_result
    c[full, 0] = max_result
    c[full, 1] = 0
    return c


def _scene(config):
    from oracle import binding as O
    from tests.util import scene_and_target
    sc, tp, tn, sizes = scene_and_target(config)
    return sc, tp, tn, sizes, O.uniform_sampling(sc.verts, 16)


def _handle(sc, nodes, tp, tn, index_base=0):
    from multiviewstitch_amd import deformation
    d = deformation.Deformation(sc.verts, sc.normals, sc.faces)
    d.set_nodes(nodes)
    d.set_target(tp, tn, index_base)
    return d


def outputs(d, graph=True) -> dict:
    """the association outputs of the handle's last pass"""
    t = d.node_targets(smoothed=False)
    out = dict(d2min=digest(t["d2min"]), top_idx=digest(t["top_idx"]), valid=digest(t["valid"]), controls=digest(t["controls"]),
               counts=digest(clamp_counts(t["counts"], d.params.max_result)))
    if graph:
        out["graph"] = digest(d.node_graph())
    return out


def _passes(d, n, tag, out, nodes=None):
    """n calls of iterate(1), every pass digested; a pass whose node positions are not finite leaves its graph out, a mesh that is not
    finite any more ends the run (as test_bounded_passes_on_odd_inputs_match_oracle)"""
    for it in range(n):
        finite = nodes is None or bool(np.isfinite(d.vertices()[nodes]).all())
        st = d.iterate(1)
        out[f"{tag}{it}"] = dict(outputs(d, graph=finite), status=int(st["status"]), n_valid=int(st["n_valid"]))
        if not np.isfinite(d.vertices()).all():
            break
    return out


def _fused(cfg):
    sc, tp, tn, _, nodes = _scene(int(cfg[1:]))
    d = _handle(sc, nodes, tp, tn)
    out = _passes(d, 1, "pass", {})
    d.close()
    return out


def _full_passes(cfg):
    sc, tp, tn, _, nodes = _scene(int(cfg[1:]))
    d = _handle(sc, nodes, tp, tn)
    out = _passes(d, 5, "pass", {})
    d.set_vertices(sc.verts, sc.normals)
    _passes(d, 3, "again", out)
    d.close()
    return out


def _odd(case):
    sc, tp, tn, _, nodes = _scene(2 if case == "top3_graph3" else 1)
    tp, tn = tp.copy(), tn.copy()
    if case == "far":
        tp += 7.0
    elif case == "one_point":
        tp, tn = tp[:1].copy(), tn[:1].copy()
    elif case == "nan":
        tn[np.random.default_rng(3).choice(len(tn), len(tn) // 10, replace=False)] = np.nan
    elif case == "five_nodes":
        nodes = nodes[:5].copy()
    from multiviewstitch_amd import deformation
    d = deformation.Deformation(sc.verts, sc.normals, sc.faces)
    d.set_nodes(nodes)
    if case == "top3_graph3":
        d.params.top_k, d.params.graph_k = 3, 3
    d.set_target(tp, tn)
    out = _passes(d, 5, "pass", {}, nodes)
    d.close()
    return out


def _full_ball(max_result="64"):
    sc, tp, tn, _, nodes = _scene(1)
    d = _handle(sc, nodes, tp, tn)
    d.params.max_result = int(max_result)
    out = {}
    for it in range(5):
        _passes(d, 1, f"pass{it}/", out)
        out[f"pass{it}/0"]["full_nodes"] = int((d.node_targets()["counts"][:, 0] >= int(max_result)).sum())
    d.close()
    return out


def _sharded():
    import torch
    from multiviewstitch_amd import dist as mdist
    dev = torch.device("cuda", 0)
    sc, tp, tn, sizes, nodes = _scene(1)
    n0 = sizes[0]
    shards = [_handle(sc, nodes, tp[:n0], tn[:n0], 0), _handle(sc, nodes, tp[n0:], tn[n0:], n0)]
    K, mr = len(nodes), shards[0].params.max_result
    d2 = [torch.empty(K, dtype=torch.float32, device=dev) for _ in shards]
    rec = torch.zeros((2, K * 8 * 48), dtype=torch.uint8, device=dev)
    cnt = torch.zeros((2, K * 2), dtype=torch.int32, device=dev)
    out = {}

    def search():
        for d, b in zip(shards, d2):
            d.assoc_dmin(b.data_ptr())
            d.sync()
        dmin = torch.minimum(d2[0], d2[1]).contiguous()
        for r, d in enumerate(shards):
            d.assoc_select(dmin.data_ptr(), rec[r].data_ptr(), cnt[r].data_ptr())
            d.sync()
        return dict(d2min=digest(dmin.cpu().numpy()), records=digest(rec.cpu().numpy()),
                    counts=[digest(clamp_counts(cnt[r].cpu().numpy(), mr)) for r in range(2)])

    def merged(got):
        for r, d in enumerate(shards):
            t = d.node_targets()
            got[f"shard{r}"] = dict(top_idx=digest(t["top_idx"]), valid=digest(t["valid"]), controls=digest(t["controls"]),
                                    graph=digest(d.node_graph()), vertices=digest(d.vertices()))
        return got

    for it in range(3):
        got = search()
        for d in shards:
            d.assoc_merge(rec.data_ptr(), cnt.data_ptr(), 2)
            d.solve()
        out[f"outer{it}"] = merged(got)
    # one owner-merges round: every rank merges its node block, the blocks are installed everywhere (k_install_targets)
    bn, blocks = mdist.node_blocks(K, 2)
    stride = (bn * 25 + 31) // 32 * 32
    blk_all = torch.zeros(2 * stride, dtype=torch.uint8, device=dev)
    got = search()
    for r, d in enumerate(shards):
        k0, k1 = blocks[r]
        rin = torch.cat([rec[s, k0 * 384:k1 * 384] for s in range(2)]).contiguous()
        cin = torch.cat([cnt[s, k0 * 2:k1 * 2] for s in range(2)]).contiguous()
        torch.cuda.synchronize()
        d.assoc_merge_block(rin.data_ptr(), cin.data_ptr(), 2, k0, k1, bn, blk_all[r * stride:].data_ptr())
        d.sync()
    for d in shards:
        d.set_node_targets_dev(blk_all.data_ptr(), 2, bn, stride)
        d.solve()
    got["blocks"] = digest(blk_all.cpu().numpy())
    out["owner_merges"] = merged(got)
    for d in shards:
        d.close()
    return out


def _group(cfg):
    from multiviewstitch_amd import _lib as L
    sc, tp, tn, sizes, nodes = _scene(int(cfg[1:]))
    n0 = sizes[0]
    hs = [_handle(sc, nodes, tp, tn), _handle(sc, nodes, tp[n0:], tn[n0:])]      # (the whole target; all views but the first)
    out = {}
    for k, d in enumerate(hs):
        _passes(d, 2, f"h{k}/alone", out)
    arr = (C.c_void_p * 2)(*[d._h for d in hs])
    g, st = C.c_void_p(), (L.CStats * 2)()
    L.check(L.lib().mvs_deform_group_create(C.cast(arr, C.c_void_p), 2, C.cast(C.byref(g), C.c_void_p)))
    rc = L.lib().mvs_deform_group_iterate(g, C.byref(hs[0].params), 0, C.cast(st, C.c_void_p))
    out["grouped"] = int(rc == 0)
    for it in range(3):
        if rc == 0:
            L.check(L.lib().mvs_deform_group_iterate(g, C.byref(hs[0].params), 1, C.cast(st, C.c_void_p)))
        for k, d in enumerate(hs):
            if rc != 0:
                d.iterate(1)
            out[f"h{k}/pass{it}"] = dict(outputs(d), vertices=digest(d.vertices()))
    L.lib().mvs_deform_group_destroy(g)
    for d in hs:
        d.close()
    return out


def _ties(where="far"):
    sc, tp, tn, _, nodes = _scene(1)
    tp, tn = tp.copy(), tn.copy()
    if where == "far":
        tp += 7.0
    # the node with the largest ball that is not full, in the third (the first bounded) pass of a run without the copies
    d = _handle(sc, nodes, tp, tn)
    for _ in range(3):
        d.iterate(1)
    t = d.node_targets()
    d.close()
    size = np.where((t["counts"][:, 0] < d.params.max_result) & (t["top_idx"][:, 0] >= 0), t["counts"][:, 0], -1)
    node = int(np.argmax(size))
    out = dict(node=node, ball=int(size[node]))
    j = int(t["top_idx"][node, 0]) if size[node] >= 0 else 0
    out["point"] = j
    tp2 = np.concatenate([tp, np.repeat(tp[j:j + 1], N_COPIES, axis=0)])
    tn2 = np.concatenate([tn, np.repeat(tn[j:j + 1], N_COPIES, axis=0)])
    d = _handle(sc, nodes, tp2, tn2)
    _passes(d, 5, "pass", out, nodes)
    d.close()
    return out


def record(case) -> dict:
    kind, *rest = case.split("/")
    if kind in ("far", "one_point", "nan", "top3_graph3", "five_nodes"):
        return _odd(kind)
    return dict(fused=_fused, passes=_full_passes, full_ball=_full_ball, sharded=lambda cfg: _sharded(), group=_group, ties=_ties)[kind](*rest)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the commit the library was built from")
    ap.add_argument("--only", nargs="+", choices=CASES, help="these cases only")
    ap.add_argument("--out", help="the file to write (default: stdout)")
    a = ap.parse_args()
    text = json.dumps(dict(parent=a.parent, cases={c: record(c) for c in (a.only or CASES)}), indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
