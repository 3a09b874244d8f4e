#!/usr/bin/env python3
"""bench.py — outer non-rigid iterations per second of the MI355X deformation engine.

One "step" = one pass of the reference's while(counter--) body
(R/Deformation/Deformation.cpp:253-401): associate all K nodes against all P target
points -> 9-NN node graph -> 2 smoothing sweeps -> ARAP(5 iterations, energy stop) ->
overwrite geometry, on BASELINE.json's metric workload (config 3: 8 views of 1280x960
inverse depth -> ~2 M target points, ~8 K nodes).  Inputs (depth rasters -> points ->
SRT map -> spatial index, template mesh) are resident in HBM before the timed region.

N > 1: one rank per GPU; views are sharded over the ranks, the template is replicated; per
step one all-reduce(MIN) + one all-gather over RCCL (multiviewstitch_amd/dist.py).  The total
work is fixed -> "scaling": "strong".  Ranks come from an external launcher
(torch.distributed.run sets RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*) or, when WORLD_SIZE is
not set and --gpus N > 1, from THIS script: the parent — before anything touches the GPU —
starts N fresh child processes of itself with those variables set, relays rank 0's JSON line
and exits non-zero if any child did.

A plain run sets up, warms up, times --steps outer iterations, writes the last step's mesh with --dump-outputs DIR and
prints ONE JSON line on rank 0.  Everything else it can measure (roofline, the reference's own call, fresh-process calls,
other schedules, solvers and tolerances, the copy ceiling, per-collective times, the CPU baseline and its parity) runs
with --full only.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=3, help="scene config (multiviewstitch_amd/scene.py); 3 = metric workload")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: roofline (HIP-event sampling inside the timed region + a pass of its own), the reference's "
                         "call on fresh handles and in fresh processes, single-solve schedule, tolerance headroom, copy ceiling, "
                         "alternative solver, per-collective times (N > 1), CPU baseline + parity; the --no-* options trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the mesh the last step left (vertices, normals, rotations; float64) as DIR/<name>.npy")
    ap.add_argument("--phases", action="store_true", help="extra instrumented pass: per-phase HIP-event times to stderr")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and its parity check")
    ap.add_argument("--no-alt-solver", action="store_true", help="skip the comparison run with the one-kernel-per-iteration CG (profiles of the default solver alone)")
    ap.add_argument("--no-single-solve", action="store_true", help="skip the run with one global solve per outer iteration (kernel-trace profiles: launches per outer iteration then count the metric's schedule only)")
    ap.add_argument("--no-tolerance-headroom", action="store_true", help="skip the runs at cg_tol 1e-7 / 1e-6 reported beside the headline")
    ap.add_argument("--no-cold-process", action="store_true", help="skip the two child processes that time the call of a fresh process (scripts/cold_call.py)")
    ap.add_argument("--only-alt-solver", action="store_true", help="time the CG solver as the main run (profiles of the CG path alone)")
    ap.add_argument("--exchange", default="auto", choices=["auto", "all_gather", "owner"],
                    help="N > 1: how the ranks' best-8 records meet (auto = all_gather at every N, as the C library's MVS_EXCHANGE_AUTO: the "
                         "owner-merges form has never run on more than one GPU; DESIGN.md §7)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only to rehearse "
                                                      "the N > 1 code path with several ranks sharing one GPU)")
    ap.add_argument("--dry-run", action="store_true", help="launcher rehearsal without a GPU: every rank joins the process group "
                                                           "(use --backend gloo), one all-reduce, rank 0 prints a JSON line")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def dry_run(args) -> int:
    """What a rank does with --dry-run: rendezvous + one collective, no GPU (tests/test_dist_gloo.py runs it on the CPU)."""
    import torch
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if os.environ.get("MVS_BENCH_FAIL_RANK") == str(rank):
        return 3                                               # rehearses a rank that dies: the parent must report it
    if world > 1:
        dist.init_process_group(args.backend, rank=rank, world_size=world)
        t = torch.tensor([float(rank + 1)])
        dist.all_reduce(t)
        total, ranks, backend = float(t.item()), dist.get_world_size(), dist.get_backend()
        dist.destroy_process_group()
    else:
        total, ranks, backend = 1.0, 1, None
    if rank == 0:
        print(json.dumps({"metric": "nonrigid_outer_iterations_per_sec", "dry_run": True, "n_gpus": world, "ranks": ranks,
                          "backend": backend, "sum_of_rank_ids_plus_1": total}), flush=True)
    return 0


# ------------------------------------------------------------------------------ launcher ----
def launch_ranks(args) -> int:
    """--gpus N > 1 without an external launcher: N children of this script, one per rank.  Runs before torch / HIP are
    imported in this process (a process that has initialised the GPU must never fork or exec workers)."""
    n = args.gpus
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    import tempfile
    procs = []
    out0 = tempfile.TemporaryFile()
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", MVS_BENCH_CHILD="1")
        # as torch.distributed.run does for its workers: without it every rank's torch / gloo host code spreads over all the
        # host's cores, N ranks oversubscribe the box's CPU share and a 32 KB gloo all-reduce takes 30-60 ms instead of 0.3
        # (two ranks on a one-GPU box: 130-170 ms per step against 3.1).  The oracle legs set their own thread count.
        env.setdefault("OMP_NUM_THREADS", "1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=out0 if r == 0 else subprocess.DEVNULL))
    # wait for all; a rank that dies takes the others down with it (they would wait for it in a collective for ever)
    codes = [None] * n
    while any(c is None for c in codes):
        for r, p in enumerate(procs):
            if codes[r] is None:
                codes[r] = p.poll()
        if any(c not in (None, 0) for c in codes):
            for r, p in enumerate(procs):
                if codes[r] is None:
                    p.terminate()                     # exactly the children started above
            for r, p in enumerate(procs):
                if codes[r] is None:
                    try:
                        codes[r] = p.wait(timeout=20)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        codes[r] = p.wait()
            break
        time.sleep(0.1)
    out0.seek(0)
    line = None
    for ln in out0.read().decode(errors="replace").splitlines():
        if ln.lstrip().startswith("{"):
            line = ln
    if line is not None and not any(codes):
        print(line, flush=True)
    if any(codes) or line is None:
        log(f"[bench] rank exit codes {codes}" + ("" if line is not None else "; rank 0 printed no JSON line"))
        return 1
    return 0


def build_target(torch, srt_mod, scene_mod, sc, views, device):
    """depth rasters -> world-frame target points + normals in HBM (engine kernels only)."""
    pts_l, nrm_l = [], []
    for k in views:
        d = torch.from_numpy(np.ascontiguousarray(sc.depth[k])).to(device)
        cam = sc.cams[k]
        npnt, _ = srt_mod.depth_to_model_dev(d.data_ptr(), cam, scene_mod.MIN_DSP, scene_mod.MAX_DSP, scene_mod.SMOOTH)
        p = torch.empty((npnt, 3), dtype=torch.float64, device=device)
        n = torch.empty((npnt, 3), dtype=torch.float64, device=device)
        srt_mod.depth_to_model_dev(d.data_ptr(), cam, scene_mod.MIN_DSP, scene_mod.MAX_DSP, scene_mod.SMOOTH,
                                   p.data_ptr(), n.data_ptr())
        s, R, t = sc.srt[k]
        pw, nw = torch.empty_like(p), torch.empty_like(n)
        srt_mod.apply_dev(p.data_ptr(), n.data_ptr(), npnt, s, R, t, pw.data_ptr(), nw.data_ptr())
        torch.cuda.synchronize(device)
        pts_l.append(pw)
        nrm_l.append(nw)
    if not pts_l:
        z = torch.zeros((0, 3), dtype=torch.float64, device=device)
        return z, z.clone()
    return torch.cat(pts_l).contiguous(), torch.cat(nrm_l).contiguous()


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.lower().startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def dump_outputs(out_dir, d):
    """What a caller of the timed path receives after its last step: the deformed mesh (float64, ~6.5 MB at config 3)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"vertices": d.vertices(), "normals": d.normals(), "rotations": d.rotations()}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    log(f"[bench] outputs of the last timed step -> {out_dir}: " + ", ".join(f"{n} {a.shape}" for n, a in arrays.items()))


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args))
    if args.dry_run:
        sys.exit(dry_run(args))

    import torch
    import torch.distributed as dist
    from multiviewstitch_amd import _lib, deformation, srt as srt_mod, scene as scene_mod
    from multiviewstitch_amd import dist as mdist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    n_dev = torch.cuda.device_count()
    dev_id = local_rank % n_dev                              # == local_rank on a full node
    torch.cuda.set_device(dev_id)
    device = torch.device("cuda", dev_id)
    _lib.check(_lib.lib().mvs_set_device(dev_id))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    # ------------------------------------------------------------------ inputs ----
    t0 = time.time()
    cfg = scene_mod.CONFIGS[args.config]
    shards = mdist.view_shards(cfg["n_views"], world)
    my_views = shards[rank]
    sc = scene_mod.make_scene(args.config, device=device, views=set(my_views))
    log(f"[bench r{rank}] scene config {args.config}: V={len(sc.verts)} F={len(sc.faces)} views={my_views} ({time.time()-t0:.1f}s)")
    d = deformation.Deformation(sc.verts, sc.normals, sc.faces, device=dev_id)
    if args.only_alt_solver:
        d.params.solver = 1
        args.no_alt_solver = True
    t1 = time.time()
    K = d.UniformSampling(16)
    tp, tn = build_target(torch, srt_mod, scene_mod, sc, my_views, device)
    P_local = tp.shape[0]
    offs, counts = mdist.exclusive_offsets(P_local, world, device)
    P_total = int(counts.sum())
    t2 = time.time()
    d.set_target_dev(tp.data_ptr(), tn.data_ptr(), P_local, int(offs[rank]))
    torch.cuda.synchronize(device)
    log(f"[bench r{rank}] K={K} nodes ({t2-t1:.2f}s incl. depth->points), P_local={P_local} P_total={P_total}, "
        f"grid build {time.time()-t2:.3f}s")

    worst = {"rel": 0.0, "missed": 0, "solves": 0, "status": 0}

    def note(st):
        if st is not None:
            worst["rel"] = max(worst["rel"], st["worst_rel_residual_in_batch"])
            worst["missed"] += st["unconverged_solves"]
            worst["solves"] += st["solves_in_batch"]
            worst["status"] = max(worst["status"], st["status"])
        return st

    exchange = shard = bufs = None
    if world > 1:
        shard = mdist.EngineShard(d, device)
        bufs = shard.buffers(K, world)
        exchange = "all_gather"
        want = args.exchange if args.exchange != "auto" else "all_gather"
        if want == "owner":
            # owner-merges exchange: checked once, before anything is timed, against the all-gather exchange on the
            # same records — identical node targets on this rank, and every rank must agree — else the all-gather form runs
            # (--exchange auto) or the bench fails (--exchange owner).  Every step a rank could decline on its own (buffer
            # allocation, the comparison) is followed by an agreement all-reduce BEFORE the next collective, so that no rank
            # ever waits in a collective its peers have left; an exception inside a collective itself is
            # fatal for the whole job, as it should be.
            def agree(ok):
                t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device)
                dist.all_reduce(t, op=dist.ReduceOp.MIN)
                return int(t.item()) == 1
            ok, why, obufs = True, "", None
            try:
                obufs = shard.buffers_owner(K, world, rank)
            except Exception as e:                          # noqa: BLE001
                ok, why = False, f"{type(e).__name__}: {e}"
            if agree(ok):
                with torch.cuda.stream(shard.stream):
                    shard.dmin(obufs)
                    dist.all_reduce(obufs["d2min"], op=dist.ReduceOp.MIN)
                    shard.select(obufs)
                    bufs["rec"].copy_(obufs["rec"]); bufs["cnt"].copy_(obufs["cnt"])
                    dist.all_gather_into_tensor(bufs["pack_all"], bufs["pack"])
                    shard.merge(bufs, world)
                torch.cuda.synchronize(device)
                a = d.node_targets()
                with torch.cuda.stream(shard.stream):
                    mdist._sharded_exchange_owner(shard, obufs, world, None, None)
                torch.cuda.synchronize(device)
                b = d.node_targets()
                same = np.array_equal(a["controls"], b["controls"]) and np.array_equal(a["valid"], b["valid"])
                if not same:
                    ok, why = False, "targets differ from the all-gather exchange"
                ok = agree(same)
            else:
                ok = False
            if ok:
                bufs, exchange = obufs, "owner_merges"
            else:
                log(f"[bench r{rank}] owner-merges exchange not used ({why or 'another rank declined'})")
                if args.exchange == "owner":
                    raise SystemExit(f"--exchange owner: the owner-merges check failed on rank {rank}: {why or 'another rank declined'}")
                exchange = "all_gather (owner-merges check failed)"

        def run(n, timers=None):
            st = None
            for k in range(n):                    # the last step synchronises with the host (and every 32nd: the solver
                st = note(mdist.sharded_step(shard, bufs, world, sync=(k == n - 1 or k % 32 == 31), timers=timers))   # re-plans, as iterate() does)
            return st
    else:
        def run(n, timers=None):
            return note(d.iterate(n))

    def fence():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    # ------------------------------------------------------------ warmup + timed ----
    # the first outer iteration of a fresh handle runs fixed first plans (7 6 5 5 5 launches per solve, trimmed or extended by the
    # device) and harvests them into the handle's launch plan: timed on its own, reported in "regime"
    fence()
    tf = time.perf_counter()
    run(1)
    fence()
    first_ms = 1e3 * (time.perf_counter() - tf)
    st = run(max(args.warmup - 1, 0)) if args.warmup > 1 else None
    if st is not None:
        log(f"[bench r{rank}] warmup done: solver iterations={st['cg_iters']} arap_iters_run={st['arap_iters_run']} "
            f"n_valid={st['n_valid']} worst rel residual of the warm-up batch={st['worst_rel_residual_in_batch']:.2e}")
    worst.update(rel=0.0, missed=0, solves=0, status=0)
    if args.full:                           # HIP events around the planned sweeps of the solves of every 8th pass (around every
        d.enable_timing(3)                  # solve they cost 5 % of the step: scripts/timing_overhead.py), for the roofline
    fence()
    tb = time.perf_counter()
    st = run(args.steps)
    fence()
    te = time.perf_counter()
    elapsed = te - tb
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    ms_per_step = 1e3 * elapsed / args.steps
    value = args.steps / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, d)
    timed = dict(worst)
    log(f"[bench r{rank}] timed batch: worst true relative residual {timed['rel']:.2e} over {timed['solves']} solves, "
        f"{timed['missed']} above cg_tol, status {timed['status']}")
    V = len(sc.verts)
    info = d.solver_info()
    extras = {}
    if args.full:
        extras = measure_full(args, d=d, sc=sc, tp=tp, tn=tn, device=device, dev_id=dev_id, run=run, fence=fence, st=st, K=K, V=V,
                              info=info, world=world, rank=rank, P_local=P_local, P_total=P_total, ms_per_step=ms_per_step,
                              shard=shard, bufs=bufs, exchange=exchange)

    if args.phases:
        d.enable_timing(1)
        run(args.steps)
        fence()
        tot = 0.0
        for name in ("assoc", "graph", "smooth", "weights", "rhs", "cg", "tail", "local", "finalize"):
            ms, n = d.kernel_time(name)
            tot += ms
            log(f"[phases r{rank}] {name:9s} {ms/args.steps:9.4f} ms/step  {n/args.steps:7.1f} launches/step")
        log(f"[phases r{rank}] sum       {tot/args.steps:9.4f} ms/step")
        d.enable_timing(0)

    if rank == 0:
        out = {
            "metric": "nonrigid_outer_iterations_per_sec", "value": round(value, 3), "unit": "iter/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "dtype_note": "fp64 geometry, right-hand sides, residuals and solution; the inexact LOCAL correction inside a patch sweep "
                          "runs in f32 with bf16 neighbour directions (the fp64 true residual decides convergence)",
            "data": "synthetic",
            "config": {"workload": f"config{args.config}: {cfg['n_views']} views {cfg['w']}x{cfg['h']} inverse depth, "
                                   f"P={P_total} target points, K={K} nodes, V={V} template vertices; step = associate + "
                                   f"9-NN graph + 2 smoothing sweeps + ARAP(5, 1e-4) + geometry update",
                       "points": P_total, "nodes": int(K), "vertices": V, "views_per_gpu": len(my_views),
                       "global_solver": info["kind"], "solver_launches_per_step": int(st["cg_launches"]),
                       "local_iters_per_step": int(st["cg_iters"]), "valid_nodes": int(st["n_valid"]),
                       "parallelism": f"views sharded x{world}, template replicated"},
            "regime": {"timed": f"outer iterations {args.warmup}..{args.warmup + args.steps - 1} of a fresh fit from the template pose",
                       "first_outer_iteration_ms": round(first_ms, 3),
                       "event_sampling_in_timed_region": bool(args.full),      # --full: the roofline's HIP events (every 8th pass)
                       "note": "fewer than half of the nodes hold a correspondence in this regime (the reference rejects nodes whose "
                               "mean direction is nearly tangential, |cos| < 0.1); past ~170 outer iterations of a fit (which the reference "
                               "never runs: counter = 1) one sliver triangle stalls the sweeps and the solver switches to Anderson-mixed "
                               "sweeps: 0.63-0.68 ms per step (profiles/r03/soak_400_outer.log, DESIGN.md §5)"},
            "solver": {"worst_rel_residual_timed": timed["rel"], "solves_timed": timed["solves"],
                       "unconverged_solves_timed": timed["missed"], "status": timed["status"], "cg_tol": d.params.cg_tol},
        }
        out.update(extras)
        if world > 1:
            out["ranks"] = dist.get_world_size()
            out["backend"] = dist.get_backend()
            out["gpus_visible"] = n_dev
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def measure_full(args, *, d, sc, tp, tn, device, dev_id, run, fence, st, K, V, info, world, rank, P_local, P_total, ms_per_step,
                 shard, bufs, exchange):
    """--full: every figure beside the headline, measured after the timed region on the same handle and inputs.  Returns the
    result-line fields it fills (the headline's own fields stay as the plain run computed them)."""
    import torch
    import torch.distributed as dist
    from multiviewstitch_amd import deformation
    # (sampled passes bracket the planned sweeps of each solve; the idle flags those very launches left are read back: "cg_idle"
    #  counts them, and every bracket is filed under its composition "cg:a<active>:i<idle>")
    cg_ms, cg_launches = d.kernel_time("cg")
    idle_n = d.kernel_time("cg_idle")[1]
    brackets = []                               # (active, idle, brackets of this composition, their total ms)
    for na in range(0, 17):
        for ni in range(0, 17):
            ms_c, n_c = d.kernel_time(f"cg:a{na}:i{ni}")
            if n_c:
                brackets.append((na, ni, int(n_c), ms_c))
    d.enable_timing(0)
    tail_ms, tail_launches = 0.0, 0
    if world == 1:                          # the last launch of every solve (decides; ARAP local step): events in a pass of its own, outside the timed region
        d.enable_timing(2)
        run(4)
        fence()
        tail_ms, tail_launches = d.kernel_time("tail")
        d.enable_timing(0)

    # ---------------------------------------------------------------- roofline ----
    # Dominant kernel = the global-solve kernel (the "cg" phase timer brackets exactly its launches).
    deg = np.bincount(sc.faces.reshape(-1), minlength=V)          # closed manifold: degree == facet count
    if info["kind"] == "patch":
        # k_ras_sweep (schwarz.hip): one launch = one overlapping-patch sweep over all V rows, 3 rhs fused.
        # Algorithmic bytes per launch: the patch tables are distinct data per patch-local row
        # (local column slot 2 + weight 8 per stored entry, l2g 4, diagonal 8), every vertex's x and b are needed once
        # (24 + 24; re-reads by the overlap rows and by the halo slots are not counted) and every vertex's x is written
        # once (24).
        kernel = "k_ras_sweep"
        solve_bytes = (10 * info["width"] + 12) * info["local_rows"] + 72 * V
    else:
        # k_cg_iter (arap.hip): one launch = one CG iteration over all V rows: every CG vector r,w,s,p,x read once and
        # written once (fp64 AoS, 24 B) + diag 8 B + ctrl id 4 B per vertex row, + 12 B (col 4, w 8) per stored entry
        # of the ELL-8-by-row-group layout (a group of 8 rows stores ceil(max degree / 8) passes of 64 entries).
        kernel = "k_cg_iter"
        n_entries = int(sum(-(-int(deg[i:i + 8].max()) // 8) * 64 for i in range(0, V, 8)))
        solve_bytes = 252 * V + 12 * n_entries
    roofline = None
    # HBM-side traffic of the same kernel from the committed rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE in
    # separate runs, gfx950 x2 fetch correction calibrated on k_srt_apply): profiles/rNN/pmc_traffic*.json (newest round wins)
    traffic, traffic_src = None, None
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_traffic*.json"))):
        try:
            t = json.load(open(f))
            if t.get("kernel") == kernel and t.get("vertices") == V:
                traffic, traffic_src = int(t["bytes_per_active_launch"]), os.path.relpath(f, ROOT)
        except Exception:
            pass
    active_per_step = st["cg_active"]
    timed_launches = int(cg_launches)
    if timed_launches > 0 and cg_ms > 0:
        # launches that found all three right-hand sides converged degenerate into a copy of the owned rows (the first one) or
        # return after one scalar load (the others): only the active ones move the algorithmic bytes.  Active and idle launches
        # are counted among the TIMED launches themselves (device flags); their costs are separated by least squares over the
        # brackets, T = a * active + b * idle + c (c = what an event pair adds to the stream, ~4 us).
        n_last = st["arap_iters_run"] if info["kind"] == "patch" else 0
        n_idle = int(idle_n)
        n_active = timed_launches - n_idle
        t_all = 1e-3 * cg_ms
        avg_s = t_all / timed_launches
        a_s, b_s, c_s, how = None, None, None, None
        if brackets:
            A = np.array([[na, ni, 1.0] for na, ni, _, _ in brackets], dtype=np.float64)
            w = np.sqrt(np.array([n_c for _, _, n_c, _ in brackets], dtype=np.float64))
            y = np.array([1e-3 * ms_c / n_c for _, _, n_c, ms_c in brackets], dtype=np.float64)      # mean bracket time per composition
            for cols in ((0, 1, 2), (0, 2), (0, 1), (0,)):                  # the fullest model the sample supports
                M = A[:, cols]
                if len(brackets) < len(cols) or np.linalg.matrix_rank(M) < len(cols):
                    continue
                sol, *_ = np.linalg.lstsq(M * w[:, None], y * w, rcond=None)
                coef = dict(zip(cols, (float(v) for v in sol)))
                if coef[0] > 0 and coef.get(1, 0.0) >= 0 and coef.get(2, 0.0) >= 0:
                    a_s, b_s, c_s = coef[0], coef.get(1), coef.get(2)
                    how = (f"weighted least squares over {len(brackets)} bracket compositions ({int((w * w).sum())} brackets): "
                           "T = " + " + ".join(t for t, k in (("a*active", 0), ("b*idle", 1), ("c", 2)) if k in cols))
                    break
        if a_s is None or not (a_s > 0):
            a_s, how = (t_all - n_idle * 2.5e-6) / max(1, n_active), "idle launches priced at 2.5 us (rocprofv3 minimum of the kernel)"
            b_s, c_s = 2.5e-6, None
        active_frac = n_active / timed_launches
        ach = active_frac * solve_bytes / avg_s / 1e9
        roofline = {"bound": "hbm", "kernel": kernel, "achieved": round(ach, 1), "peak": 8000.0, "unit": "GB/s",
                    "frac": round(ach / 8000.0, 4),
                    "frac_active": round(solve_bytes / a_s / 1e9 / 8000.0, 4) if a_s else None,
                    "traffic": traffic, "traffic_source": traffic_src,
                    "bytes_per_launch": solve_bytes,
                    "avg_launch_us": round(1e6 * avg_s, 3), "launches": timed_launches, "active_fraction": round(active_frac, 3),
                    "active_launches": n_active, "avg_active_launch_us": round(1e6 * a_s, 3) if a_s else None,
                    "idle_launches": n_idle, "avg_idle_launch_us": round(1e6 * b_s, 3) if b_s is not None else None,
                    "bracket_overhead_us": round(1e6 * c_s, 3) if c_s is not None else None,
                    "brackets": [{"active": na, "idle": ni, "n": n_c, "mean_us": round(1e3 * ms_c / n_c, 3)} for na, ni, n_c, ms_c in brackets],
                    "separation": how,
                    "launches_per_step": int(st["cg_launches"]),
                    "timed_sample": "the planned sweep launches of every 8th outer iteration of the timed region (HIP events on the engine's "
                                    "stream); active / idle counted from the idle flags those launches left on the device",
                    "share_of_step": round(1e3 * (avg_s * (st["cg_launches"] - n_last) + (1e-3 * tail_ms / tail_launches * n_last if tail_launches else 0.0)) / ms_per_step, 3)}
        if tail_launches:
            roofline["last_launch_of_a_solve"] = {"kernel": "k_ras_sweep<W, 2> (decides the solve; ARAP local step on the owned rows)",
                                                  "avg_launch_us": round(1e3 * tail_ms / tail_launches, 3), "per_step": int(n_last)}
        if info["kind"] == "patch":
            roofline["note"] = ("LDS-resident local iterations: the launch is bound by its dependent load chain and workgroup "
                                "barriers, not by HBM bytes; local Chebyshev steps per active launch = "
                                f"{st['cg_iters'] / max(1, st['cg_active']):.1f}; idle launches (solve finished) return after one scalar load")
        # the whole iteration against the HBM roof, B_iter = 24 P + 328 K + 264 V + n_cg * 108 V (its fp32 /
        # int32 storage model) with the solver passes actually run per step
        b_iter = 24 * P_total + 328 * int(K) + 264 * V + int(active_per_step) * 108 * V
        roofline["step"] = {"bytes": int(b_iter), "solver_passes": int(active_per_step),
                            "achieved": round(b_iter / (1e-3 * ms_per_step) / 1e9, 1), "unit": "GB/s",
                            "frac": round(b_iter / (1e-3 * ms_per_step) / 1e9 / 8000.0, 4),
                            "formula": "SURVEY 8(d): 24P + 328K + 264V + n_cg*108V"}

    # ------------------------------------------------------------------ the reference's own call ----
    # Processor::Deform builds a FRESH Deformation, samples the nodes and calls Deform once (counter = 1):
    # R/Processor/Processor.cpp:1135-1136, R/Deformation/Deformation.cpp:248-253,398.  Timed here exactly so — create +
    # sample_nodes + set_target (spatial index) + ONE outer iteration (ARAP(5, 1e-4)) + read-back of the vertices — on a fresh
    # handle each time, host wall clock around each C-ABI call (each returns synchronised except create, which is followed by
    # a sync of its own here), target already in HBM.  `first` still pays the one-off loading of the set-up kernels' code.
    ref_sched = None
    if world == 1:
        reps = []
        for rep in range(4):
            torch.cuda.synchronize(device)
            c0 = time.perf_counter()
            d2 = deformation.Deformation(sc.verts, sc.normals, sc.faces, device=dev_id)
            d2.sync()
            c1 = time.perf_counter()
            K2 = d2.UniformSampling(16)
            d2.sync()
            c2 = time.perf_counter()
            d2.set_target_dev(tp.data_ptr(), tn.data_ptr(), P_local, 0)
            c3 = time.perf_counter()
            st2 = d2.iterate(1)
            c4 = time.perf_counter()
            v2 = d2.vertices()
            c5 = time.perf_counter()
            reps.append([1e3 * (b - a) for a, b in ((c0, c1), (c1, c2), (c2, c3), (c3, c4), (c4, c5), (c0, c5))])
            assert K2 == K and st2["status"] == 0 and np.isfinite(v2).all()
            d2.close()
        best = min(reps[1:], key=lambda r: r[5])
        names = ("create", "sample_nodes", "set_target_dev", "iterate_1", "get_vertices")
        ref_sched = {"gpu_ms": round(best[5], 3), "phases_ms": {n: round(best[i], 3) for i, n in enumerate(names)},
                     "first_rep_ms": round(reps[0][5], 3), "reps": len(reps),
                     "what": "fresh handle: mvs_deform_create + sample_nodes(16) + set_target_dev + iterate(1) [1 outer x ARAP(5, 1e-4)] + "
                             "get_vertices; best of the reps after the first; R/Processor/Processor.cpp:1135-1136"}
        log(f"[bench] reference schedule on a fresh handle: {ref_sched['gpu_ms']} ms {ref_sched['phases_ms']} (first rep {ref_sched['first_rep_ms']} ms)")
        # ... and in a FRESH PROCESS, which is what the reference's own process is (R/main.cpp:24-25 calls Processor::Deform once):
        # scripts/cold_call.py, a child of this process, twice — the call after the library's cold-start helper thread has finished
        # (code objects loaded, first stream created: a host that reads its input files in between), and the call at once.
        if not args.no_cold_process:
            cold = {}
            for mode in ("wait", "immediate"):
                try:
                    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "cold_call.py"), mode], capture_output=True, text=True, timeout=180,
                                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
                    line = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("{")]
                    cold[mode] = json.loads(line[-1]) if r.returncode == 0 and line else {"error": (r.stderr or "no output")[-300:]}
                except Exception as e:                          # noqa: BLE001
                    cold[mode] = {"error": f"{type(e).__name__}: {e}"}
            ref_sched["fresh_process"] = cold
            ref_sched["fresh_process_note"] = ("first call of a new process; 'wait_for_helper_thread_ms' = what was left of the code-object loads + the first "
                                               "stream's creation when the host asked (they start at mvs_set_device, on a helper thread)")
            log(f"[bench] fresh process: {cold}")

    # the iteration with ONE global solve per outer pass, next to the reference's own schedule
    # (ARAP(5, 1e-4), the timed step above); and the box's device-to-device streaming-copy ceiling.
    single = None
    copy_gbps = None
    alt = None
    headroom = []
    if world == 1:
        if not args.no_single_solve:
            keep = d.params.arap_iters
            d.params.arap_iters = 1
            run(max(args.warmup, 1))
            fence()
            ta = time.perf_counter()
            run(args.steps)
            fence()
            el1 = time.perf_counter() - ta
            d.params.arap_iters = keep
            single = {"ms_per_step": round(1e3 * el1 / args.steps, 4), "iter_per_s": round(args.steps / el1, 2)}
        if not args.no_tolerance_headroom:
            # the same window (a fresh fit, outer iterations warmup..warmup+steps-1) at looser solve tolerances —
            # reported BESIDE the headline, which stays at the default cg_tol = 1e-8 (profiles/r04/tolerance_headroom.md)
            for tol in (1e-7, 1e-6):
                dh = deformation.Deformation(sc.verts, sc.normals, sc.faces, device=dev_id)
                dh.params.cg_tol = tol
                dh.set_nodes(d.nodes())
                dh.set_target_dev(tp.data_ptr(), tn.data_ptr(), P_local, 0)
                dh.iterate(1)
                if args.warmup > 1:
                    dh.iterate(args.warmup - 1)
                fence()
                ta = time.perf_counter()
                sth = dh.iterate(args.steps)
                fence()
                elh = time.perf_counter() - ta
                headroom.append({"cg_tol": tol, "ms_per_step": round(1e3 * elh / args.steps, 4), "solver_launches_per_step": int(sth["cg_launches"]),
                                 "worst_rel_residual": sth["worst_rel_residual_in_batch"], "unconverged_solves": int(sth["unconverged_solves"])})
                dh.close()
        a = torch.empty(1 << 27, dtype=torch.float64, device=device).normal_()        # 1 GiB each way
        b = torch.empty_like(a)
        for _ in range(3):
            b.copy_(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize(device)
        copy_gbps = 10 * 2 * a.numel() * 8 / (1e-3 * e0.elapsed_time(e1)) / 1e9
        del a, b
        if roofline is not None:
            roofline["copy_ceiling_GBps"] = round(copy_gbps, 1)
            roofline["frac_of_copy_ceiling"] = round(roofline["achieved"] / copy_gbps, 4)
        run(1)                                # launch plan back on the 5-iteration schedule
        if info["kind"] == "patch" and not args.no_alt_solver:
            # the same step with the one-kernel-per-iteration CG (params.solver = MVS_SOLVER_CG), for comparison: its
            # kernel moves more bytes per second, the step takes twice as long
            d.params.solver = 1
            run(max(args.warmup, 1))
            d.enable_timing(2)
            fence()
            ta = time.perf_counter()
            st_cg = run(args.steps)
            fence()
            el2 = time.perf_counter() - ta
            ms2, l2 = d.kernel_time("cg")
            d.enable_timing(0)
            n_entries = int(sum(-(-int(deg[i:i + 8].max()) // 8) * 64 for i in range(0, V, 8)))
            cgb = 252 * V + 12 * n_entries
            af = st_cg["cg_active"] / max(1, st_cg["cg_launches"])
            alt = {"solver": "cg", "ms_per_step": round(1e3 * el2 / args.steps, 4), "kernel": "k_cg_iter",
                   "avg_launch_us": round(1e3 * ms2 / max(1, l2), 3), "launches_per_step": int(st_cg["cg_launches"]),
                   "achieved_GBps": round(af * cgb / (1e-3 * ms2 / max(1, l2)) / 1e9, 1),
                   "frac": round(af * cgb / (1e-3 * ms2 / max(1, l2)) / 1e9 / 8000.0, 4),
                   "worst_rel_residual": st_cg["worst_rel_residual_in_batch"]}
            d.params.solver = 0
            run(1)

    # per-collective time of the sharded step: an instrumented pass AFTER the timed region (events on the shard's stream
    # around each collective; with gloo the collective is a host round trip and the stream is drained around it)
    collectives = None
    if world > 1:
        timers = {"all_reduce": [], "all_gather": [], "sync": args.backend != "nccl"}
        d.enable_timing(1)                                    # per-phase events on this rank's stream (instrumented pass only)
        run(min(args.steps, 10), timers=timers)
        fence()
        collectives = {"backend": args.backend, "steps": min(args.steps, 10)}
        # what sharding buys: every rank's association time (its own views only) next to its replicated solve
        mine = torch.tensor([d.kernel_time("assoc")[0], d.kernel_time("cg")[0] + d.kernel_time("tail")[0] + d.kernel_time("rhs")[0] + d.kernel_time("local")[0]],
                            dtype=torch.float64, device=device) / min(args.steps, 10)
        every = torch.zeros(2 * world, dtype=torch.float64, device=device)
        dist.all_gather_into_tensor(every, mine)
        d.enable_timing(0)
        every = every.cpu().numpy().reshape(world, 2)
        collectives["assoc_ms_per_step_by_rank"] = [round(float(x), 4) for x in every[:, 0]]
        collectives["solve_ms_per_step_by_rank"] = [round(float(x), 4) for x in every[:, 1]]
        for name in ("all_reduce", "all_gather"):
            ms = [a.elapsed_time(b) if hasattr(a, "elapsed_time") else 1e3 * (b - a) for a, b in timers[name]]
            collectives[name + "_ms_per_step"] = round(float(np.mean(ms)), 4) if ms else None
        collectives["bytes_all_reduce"] = int(K) * 4
        collectives["exchange"] = exchange
        if exchange == "owner_merges":          # "all_gather" timer = all-to-all (records, counts) + block merge + all-gather of the targets
            collectives["all_gather_ms_covers"] = "all-to-all of records and counts by node block + merge of the owned block + all-gather of the merged targets"
            collectives["bytes_all_to_all_in_per_rank"] = int(K) * 392
            collectives["bytes_all_gather_in_per_rank"] = int(bufs["owner"]["stride"]) * world
        else:
            collectives["bytes_all_gather_in_per_rank"] = int(K) * 392 * world

    # ------------------------------------------------- CPU baseline + parity of this very workload ----
    cpu_baseline = None
    parity = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import binding as O
        tph, tnh = tp.cpu().numpy(), tn.cpu().numpy()
        # the reference's own call on the CPU (oracle/, one thread): constructor + UniformSampling + kd-tree build + one Deform pass
        tk0 = time.perf_counter()
        o = O.Deform(sc.verts, sc.normals, sc.faces)
        tk1 = time.perf_counter()
        Ko = o.sample_nodes(16)
        tk2 = time.perf_counter()
        assert Ko == K and np.array_equal(o.nodes(), d.nodes())
        tk = time.perf_counter()
        o.set_target(tph, tnh)                                   # kd-tree build: not part of an iteration
        t_build = time.perf_counter() - tk
        p = O.Params.default()
        if ref_sched is not None:
            o1 = O.Deform(sc.verts, sc.normals, sc.faces)
            o1.set_nodes(d.nodes())
            o1.set_target(tph, tnh)
            tk3 = time.perf_counter()
            o1.iterate(p, 1)
            t_it = time.perf_counter() - tk3
            del o1
            ref_sched["cpu_ms"] = round(1e3 * ((tk1 - tk0) + (tk2 - tk1) + t_build + t_it), 1)
            ref_sched["cpu_phases_ms"] = {"create": round(1e3 * (tk1 - tk0), 1), "sample_nodes": round(1e3 * (tk2 - tk1), 1),
                                          "set_target_kdtree": round(1e3 * t_build, 1), "iterate_1": round(1e3 * t_it, 1)}
            ref_sched["cpu_kind"] = "port (oracle/, 1 thread; its global solve is Jacobi-CG, not the reference's factor-once SparseLU)"
        # the SAME outer iterations the GPU was timed on: `warmup` untimed iterations from the template pose, then the timed
        # sample (bounded: <= steps iterations and ~12 s).  After the warm-up the oracle's mesh is compared with a fresh
        # engine handle taken through the same iterations: the parity figure of this exact workload.
        fresh = deformation.Deformation(sc.verts, sc.normals, sc.faces, device=dev_id)
        fresh.set_nodes(d.nodes())
        fresh.set_target_dev(tp.data_ptr(), tn.data_ptr(), P_local, 0)
        loose = []
        for hr in headroom:
            fh = deformation.Deformation(sc.verts, sc.normals, sc.faces, device=dev_id)
            fh.params.cg_tol = hr["cg_tol"]
            fh.set_nodes(d.nodes())
            fh.set_target_dev(tp.data_ptr(), tn.data_ptr(), P_local, 0)
            loose.append([fh, True])
        same = True
        for _ in range(max(args.warmup, 1)):
            so, sg = o.iterate(p, 1), fresh.iterate(1)
            same = same and so["n_valid"] == sg["n_valid"] and so["arap_iters_run"] == sg["arap_iters_run"]
            for lf in loose:
                sl = lf[0].iterate(1)
                lf[1] = lf[1] and so["n_valid"] == sl["n_valid"] and so["arap_iters_run"] == sl["arap_iters_run"]
        for hr, lf in zip(headroom, loose):
            dvl = lf[0].vertices() - o.vertices()
            hr["vertex_rms_vs_oracle"] = float(np.sqrt((dvl * dvl).sum(1).mean()))
            hr["integer_stats_equal"] = bool(lf[1])
            hr["after_outer"] = max(args.warmup, 1)
            lf[0].close()
        dv = fresh.vertices() - o.vertices()
        dr = (fresh.rotations() - o.rotations()).reshape(-1, 9)
        parity = {"vertex_rms_vs_oracle": float(np.sqrt((dv * dv).sum(1).mean())), "rotation_rms_vs_oracle": float(np.sqrt((dr * dr).sum(1).mean())),
                  "after_outer": max(args.warmup, 1), "integer_stats_equal": bool(same), "bound": 1e-4}
        fresh.close()
        n_it, t_cpu = 0, 0.0
        while n_it < args.steps and t_cpu < 12.0:
            ta = time.perf_counter()
            o.iterate(p, 1)
            t_cpu += time.perf_counter() - ta
            n_it += 1
        cpu_baseline = {"value": round(n_it / t_cpu, 4), "unit": "iter/s", "cores": 1, "kind": "port",
                        "cpu_model": cpu_model(), "host_cores": os.cpu_count(),
                        "note": "kind 'port' = oracle/ (this build's C++ restatement, Jacobi-CG global solve to 1e-14), not the reference's "
                                "factor-once SparseLU: it understates what the reference does per iteration",
                        "sample": f"outer iterations {max(args.warmup, 1)}..{max(args.warmup, 1) + n_it - 1} of the full workload "
                                  f"(the iterations the GPU value is timed on; oracle/, single thread as the reference, "
                                  f"kd-tree build {t_build:.2f}s excluded)"}
        # second column: the same code with OpenMP on every host core — per-node / per-vertex loops on all
        # threads, the global solve on 3 (one per right-hand side); bit-identical results
        # (one thread per core up to 32: beyond that the 8 K-node / 55 K-vertex loops are too short to amortise the fork-join)
        threads = int(os.environ.get("MVS_BENCH_OMP_THREADS", "0")) or max(1, min(32, len(os.sched_getaffinity(0))))
        O.set_threads(threads)
        n2, t2 = 0, 0.0
        while n2 < args.steps and t2 < 8.0:
            ta = time.perf_counter()
            o.iterate(p, 1)
            t2 += time.perf_counter() - ta
            n2 += 1
        O.set_threads(1)
        cpu_baseline["openmp_all_cores"] = {"value": round(n2 / t2, 4), "threads": threads, "solve_threads": min(3, threads),
                                            "sample": f"the next {n2} outer iterations"}
        log(f"[bench] cpu_baseline: {n_it} it in {t_cpu:.2f}s single thread, {n2} it in {t2:.2f}s on {threads} threads ({cpu_model()})")

    extras = {"roofline": roofline, "cpu_baseline": cpu_baseline, "parity": parity}
    if world > 1:
        extras["collectives"] = collectives
    if ref_sched is not None:
        extras["reference_schedule"] = ref_sched        # the call the reference makes: fresh Deformation + UniformSampling + one Deform
    if headroom:
        extras["tolerance_headroom"] = {"rows": headroom, "headline_cg_tol": d.params.cg_tol,
                                        "note": "the same window at looser solve tolerances, beside the headline (which is measured at the default 1e-8); integers = n_valid and "
                                                "arap_iters_run of every compared iteration; 25-iteration tables for configs 1-4: profiles/r04/tolerance_headroom.md"}
    if single is not None:
        extras["single_solve_schedule"] = single       # one ARAP global+local pass per outer iteration
    if alt is not None:
        extras["alt_solver"] = alt
    return extras


if __name__ == "__main__":
    main()
