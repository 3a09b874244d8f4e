"""First timing of the chain refinement on the GPU (csrc/srt_refine.hip) at the mvs_point_sample scale of the README: 8 sequences x about
38 000 oriented points of a synthetic closed body (a bumpy sphere; sequence k holds the samples of a lattice of its own within 75
degrees of its viewing direction, in a frame of its own), the input chain the truth perturbed by 1 degree, 0.01 and 1 % per moving
sequence, rel_dist 0.02.

The script is a driver: the step that uses the GPU is a child process under its own time limit, and a step that fails or runs out of time
ends the run.
  gpu    mvs_test_srt_refine_timed: the search-and-sum launch alone between HIP events (--reps launches after a warm one), once per form
         of the reduction of the 121 sums (a butterfly per term; LDS atomics), their sums compared; the host solve of I7 on those sums;
         the set-up (I2 and the eight grids); the whole call mvs_srt_refine_dev on resident points (host clock, the second of two
         calls) and its history; beside them, in the same process, mvs_part_recog_dev with each sequence as the template and the points
         of the seven others, mapped into its frame, as the queries: the same walk over the same number of queries without the
         gathers and sums (its own grid build and its wait are inside); and the restatement (tests/ref_srt_refine.py) for ONE pair on
         the host
It prints one JSON line and, with --md, writes the table of profiles/r34/srt_refine.md.  No time is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 500                                                               # seconds for the step


def radius(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return 1.0 + 0.08 * np.sin(3 * x) * np.cos(2 * y) + 0.05 * np.cos(4 * z) * x + 0.04 * np.sin(5 * y)


def body(d):
    """points of the bumpy sphere along the unit directions d and their unit normals (the gradient of |p| - radius(p / |p|), by central
    differences)"""
    P = d * radius(d)[:, None]
    F = lambda q: np.linalg.norm(q, axis=1) - radius(q / np.linalg.norm(q, axis=1, keepdims=True))
    e = 1e-6
    g = np.stack([(F(P + e * np.eye(3)[c]) - F(P - e * np.eye(3)[c])) / (2 * e) for c in range(3)], axis=1)
    return P, g / np.linalg.norm(g, axis=1, keepdims=True)


def build(a):
    from tests import srt_refine_scenes as SC
    m = int(a.points / 0.37)                                              # a cap of 75 degrees holds (1 - cos 75) / 2 of the sphere
    pts, nrm, world, true = [], [], [], []
    for k in range(a.seqs):
        i = np.arange(m) + 0.5
        ph, th = np.arccos(1 - 2 * i / m), np.pi * (1 + 5 ** 0.5) * i + 0.37 * k
        d = np.stack([np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph)], axis=1) @ SC._rot((1, 2, 3), 11.0 * k).T
        ang = 2 * np.pi * k / a.seqs
        view = np.array([np.cos(ang), np.sin(ang), 0.3 * np.cos(2 * ang)])
        d = d[d @ (view / np.linalg.norm(view)) > np.cos(np.radians(75.0))]
        P, N = body(d)
        last = k == a.seqs - 1
        s, Rm, t = (1.0, np.eye(3), np.zeros(3)) if last else (1.0 + 0.05 * k, SC._rot((k + 1, 2, -1), 20.0 * k + 5), np.array([0.1 * k, -0.2, 0.05 * k]))
        p, n = SC._own(P, N, s, Rm, t)
        pts.append(np.ascontiguousarray(p))
        nrm.append(np.ascontiguousarray(n))
        world.append(P)
        true.append((s, Rm, t))
    rng = np.random.default_rng(1)
    scales, Rs, ts = [], [], []
    for k, (s, Rm, t) in enumerate(true):
        if k == a.seqs - 1:
            dg, dR, dt = 1.0, np.eye(3), np.zeros(3)
        else:
            dg, dR, dt = 1.0 + 0.01 * (-1) ** k, SC._rot(rng.normal(size=3), 1.0), 0.01 * rng.normal(size=3) / 3 ** 0.5
        scales.append(dg * s)
        Rs.append(dR @ Rm)
        ts.append(dg * dR @ t + dt)
    return dict(points=pts, normals=nrm, world=world, scales=np.array(scales), Rs=np.array(Rs), ts=np.array(ts))


def step_gpu(a):
    import torch
    from multiviewstitch_amd import _lib as L, processor as P
    from tests import ref_srt_refine as R, srt_refine_scenes as SC
    sc = build(a)
    n, lib = a.seqs, L.lib()
    prm = P.srt_refine_params(rel_dist=a.rel_dist)
    pts, nrm = np.ascontiguousarray(np.concatenate(sc["points"])), np.ascontiguousarray(np.concatenate(sc["normals"]))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in sc["points"]])
    s, Rm, t = (np.ascontiguousarray(sc[k], np.float64) for k in ("scales", "Rs", "ts"))
    res = dict(step="gpu", seqs=n, points=[int(len(p)) for p in sc["points"]], rel_dist=a.rel_dist, reps=a.reps, forms={})
    sums = {}
    for rnd in range(2):                                                  # the forms in turn, twice
        for form, name in ((0, "butterfly"), (1, "lds_atomic")):
            out, cD, ms = np.zeros((n, n, R.TERMS), np.int64), np.zeros(4), np.zeros(3)
            L.check(lib.mvs_test_srt_refine_timed(L.ptr(pts), L.ptr(nrm), L.ptr(off), n, L.ptr(s), L.ptr(Rm), L.ptr(t), C.byref(prm), L.ptr(out), L.ptr(cD),
                                                  form, a.reps, L.ptr(ms)))
            sums[name] = out
            f = res["forms"].setdefault(name, dict(launch_ms=[], solve_ms=[], setup_ms=[]))
            f["launch_ms"].append(float(ms[0])); f["solve_ms"].append(float(ms[1])); f["setup_ms"].append(float(ms[2]))
    res["forms_identical"] = bool(np.array_equal(sums["butterfly"], sums["lds_atomic"]))
    cnt = sums["butterfly"][:, :, 0]
    res.update(queries=int(sum(len(p) for p in sc["points"]) * (n - 1)), accepted=int(cnt.sum()), pairs_with_matches=int((cnt > 0).sum()), D=float(cD[3]))
    # the whole call on resident points
    st = torch.cuda.current_stream()
    dp, dn = [torch.from_numpy(p).cuda() for p in sc["points"]], [torch.from_numpy(p).cuda() for p in sc["normals"]]
    call_s = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = P.RefineSRT(dp, dn, sc["scales"], sc["Rs"], sc["ts"], prm, stream=st.cuda_stream)
        call_s.append(time.perf_counter() - t0)
    res.update(call_s=call_s, iters_done=got[3]["iters_done"], history=got[3]["history"].tolist(),
               rms_to_truth=[SC.rms_to_truth(sc, sc["scales"], sc["Rs"], sc["ts"]), SC.rms_to_truth(sc, got[0], got[1], got[2])])
    # the yardstick: the same walk without the gathers and sums
    labels = [torch.zeros(len(p), dtype=torch.int32, device="cuda") for p in sc["points"]]
    qs = []
    for b in range(n):
        q = []
        for k in range(n):
            if k != b:
                sr, Rr, tr = R.relative(sc["scales"][b], sc["Rs"][b], sc["ts"][b], sc["scales"][k], sc["Rs"][k], sc["ts"][k])
                q.append(torch.from_numpy(np.ascontiguousarray(R.seq_apply(sr, Rr, tr, sc["points"][k]))).cuda())
        qs.append(torch.cat(q).contiguous())
    outs = [torch.empty(len(q), dtype=torch.int32, device="cuda") for q in qs]

    def recog():
        for b in range(n):
            L.check(lib.mvs_part_recog_dev(L.ptr(dp[b]), L.ptr(labels[b]), len(sc["points"][b]), L.ptr(qs[b]), len(qs[b]), L.ptr(outs[b])))
    recog()
    rec = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recog()
        torch.cuda.synchronize()
        rec.append((time.perf_counter() - t0) * 1e3)
    res.update(part_recog_ms=rec, part_recog_queries=int(sum(len(q) for q in qs)))
    # the restatement, one pair
    t0 = time.perf_counter()
    c, D = R.frame(sc["points"], sc["scales"], sc["Rs"], sc["ts"])
    m = R.pair_matches(sc["points"], sc["normals"], sc["scales"], sc["Rs"], sc["ts"], 0, 1, c, D, R.params(rel_dist=a.rel_dist))
    S = R.pair_sums(m)
    res.update(restatement_pair_s=time.perf_counter() - t0, restatement_pair_identical=bool(np.array_equal(np.array(S, np.int64), sums["butterfly"][0, 1])))
    return res


def write_md(path, g):
    lo = lambda v: f"{', '.join(f'{m:.3f}' for m in v)} ms; best {min(v):.3f} ms"
    bf, la = g["forms"]["butterfly"], g["forms"]["lds_atomic"]
    lines = ["| quantity | value |", "|---|---|",
             f"| shape | {g['seqs']} sequences of {min(g['points'])} to {max(g['points'])} points, rel_dist {g['rel_dist']}, D = {g['D']:.4f}; {g['queries']} queries "
             f"over {g['seqs'] * (g['seqs'] - 1)} ordered pairs, {g['accepted']} accepted matches in {g['pairs_with_matches']} pairs |",
             f"| search-and-sum launch, a butterfly per term (HIP events, {g['reps']} launches, two rounds in turn) | {lo(bf['launch_ms'])} |",
             f"| search-and-sum launch, LDS atomics of every accepted lane | {lo(la['launch_ms'])} |",
             f"| both forms give the same sums | {g['forms_identical']} |",
             f"| host solve of I7 ({7 * (g['seqs'] - 1)} unknowns, host clock) | {lo(bf['solve_ms'] + la['solve_ms'])} |",
             f"| set-up: uploads, I2, the {g['seqs']} grids (host clock, synchronised) | {lo(bf['setup_ms'] + la['setup_ms'])} |",
             f"| mvs_srt_refine_dev, the whole call on resident points (host clock, first and second call) | {g['call_s'][0] * 1e3:.1f} ms, {g['call_s'][1] * 1e3:.1f} ms; "
             f"{g['iters_done']} iterations |",
             f"| rms distance to the truth before / after | {g['rms_to_truth'][0]:.6f} / {g['rms_to_truth'][1]:.6f} |",
             f"| history (matches, rms residual) | {'; '.join(f'{int(h[0])}, {h[1]:.3e}' for h in g['history'])} |",
             f"| mvs_part_recog_dev, {g['seqs']} calls, {g['part_recog_queries']} queries in all, grid builds and waits inside (host clock) | {lo(g['part_recog_ms'])} |",
             f"| the restatement, ONE pair on the host | {g['restatement_pair_s']:.1f} s; its sums equal the launch's: {g['restatement_pair_identical']} |"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--points", type=int, default=38000, help="points per sequence, about")
    ap.add_argument("--rel-dist", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", choices=("gpu",), help="run the step in this process (the driver starts it)")
    ap.add_argument("--md", help="write the table to this file")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step_gpu(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu", "--seqs", str(a.seqs), "--points", str(a.points), "--rel-dist", str(a.rel_dist),
           "--reps", str(a.reps)]
    try:
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(failed="gpu", why=f"no result within {LIMIT} s")))
        return 1
    if run.returncode != 0:
        print(json.dumps(dict(failed="gpu", rc=run.returncode, stderr=run.stderr[-2000:])))
        return 1
    res = json.loads(run.stdout.strip().splitlines()[-1])
    if a.md:
        write_md(a.md, res)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
