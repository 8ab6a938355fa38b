#!/usr/bin/env python3
"""bench.py — NuScenes scenes/s through voxelise -> MeanVFE -> VoxelResBackBone8x on MI355X.

Contract (see the task statement): `python bench.py --gpus N --steps K --warmup W`; for N > 1 the
driver launches it under torch.distributed.run, one rank per GPU.  A step = one pass of the hot
path over one batch of B synthetic 30k-point scenes already resident in HBM (workload =
BASELINE.json configs[1]).  Scenes shard across ranks with no data-path collective (weak scaling).
The timed step (--launch graphs, default) is replayed from two captured hipGraphs with the dominant kernel's
four launches issued as plain launches between them, each bracketed with HIP events (`config.launch` says
which form ran; --launch stream issues every kernel as a plain launch).
Rank 0 prints ONE JSON line with the whole-job scenes/s plus:
  roofline     — the dominant kernel's algorithmic bytes per launch (SURVEY.md §8d formula, counts
                 taken from this run's rulebooks) / its mean launch duration measured with HIP
                 events on the launch stream, against the 8 TB/s HBM peak;
  cpu_baseline — oracle/ (CPU restatement, "port") timed on this host, 1 thread, bounded sample.
A plain run times ONE region of exactly --steps steps.  --full adds what takes runs of its own: five
repetitions of the region (`value` = the median one), the measured HBM traffic of the dominant kernel
(two rocprofv3 --pmc child passes), batch_sweep, pipelined, the secondary child processes and
cpu_baseline.  --dump-outputs DIR writes what the last timed step returned (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128, help="scenes per step per GPU (round 4: 128 — the same code gives +3.8 %% over 64 on one box: "
                                                            "the per-launch tails of 59 launches are paid once per twice the rows; 64 stays in batch_sweep)")
    ap.add_argument("--graph", action="store_true", help="replay the forward from a captured hipGraph (small batches "
                                                          "are launch-bound); per-kernel events are not recorded")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--full", action="store_true", help="also measure what takes runs of its own (see the module docstring); "
                                                         "a plain run does the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the outputs of the last one "
                                                                        "to DIR/<name>.npy (f32 / f64, a seeded sample of rows)")
    ap.add_argument("--cpu-scenes", type=int, default=8, help="--full: scenes timed through the CPU oracle on ONE thread (0 = skip the CPU baseline)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the all-core CPU leg (0 = every core this job may use: "
                                                              "min(physical cores, sched_getaffinity, cgroup cpu.max))")
    ap.add_argument("--reps", type=int, default=None, help="repetitions of the timed K-step region; `value` is the median one, the list is "
                                                           "reported (default 1, 5 with --full)")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the secondary measurements (fp32 engine, Box Seeker, extraction, "
                                                                "training step: each a fresh child process)")
    ap.add_argument("--secondary-budget", type=float, default=540.0, help="wall-clock seconds all secondary child processes may take together; "
                                                                          "those that do not fit are skipped and say so")
    ap.add_argument("--no-events", action="store_true", help="do not bracket conv launches with events")
    ap.add_argument("--launch", default="pipeline", choices=["pipeline", "graphs", "stream"],
                    help="how a timed step is issued: 'pipeline' (round 6, the batch path's default: VoxelResBackBone8x.forward_points_iter) = "
                         "--in-flight batches in flight, each replayed from two captured hipGraphs on its slot's stream with the dominant "
                         "kernel's four launches issued as plain launches between them, each bracketed with HIP events; every step's outputs "
                         "are taken inside the timed region; 'graphs' = the same two-graph replay, one batch at a time (rounds 3-5's timed "
                         "step); 'stream' = every kernel a plain stream launch (rounds 1-3's)")
    ap.add_argument("--in-flight", type=int, default=2, help="batches in flight of --launch pipeline")
    ap.add_argument("--no-traffic", action="store_true", help="--full: do not measure roofline.traffic (two rocprofv3 --pmc child runs of this "
                    "script, ~1 min); the committed profile's value is quoted then, as in a plain run")
    ap.add_argument("--no-sweep", action="store_true", help="--full: skip the extra small-batch measurements (1 and 8 scenes per step)")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 5 if args.full else 1
    return args


def algorithmic_bytes(tag, P, n_out, b):
    """P*(Cin*b + 8) + N_out*Cout*b + K*Cin*Cout*b (+ N_out*Cout*b residual read)."""
    cin, cout, K, res = tag[:4]
    v = P * (cin * b + 8) + n_out * cout * b + K * cin * cout * b
    if res:
        v += n_out * cout * b
    return v


def cgroup_cpus():
    """cores the cgroup's CPU quota allows (cpu.max = "<quota> <period>" | "max <period>"), None when unlimited / unknown"""
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] == "max":
                    return None
                return max(1, int(int(txt[0]) / int(txt[1])))
            q = int(txt[0])
            if q <= 0:
                return None
            return max(1, q // int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read()))
        except Exception:
            continue
    return None


def host_cpu():
    """CPU model, physical cores (sockets x cores per socket) and the cores this process may use."""
    import subprocess
    model, phys = "unknown", None
    try:
        txt = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = {l.split(":", 1)[0].strip(): l.split(":", 1)[1].strip() for l in txt.splitlines() if ":" in l}
        model = kv.get("Model name", model)
        phys = int(kv["Socket(s)"]) * int(kv["Core(s) per socket"])
    except Exception:
        pass
    usable = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = cgroup_cpus()
    if quota is not None:
        usable = min(usable, quota)
    return model, phys or usable, usable


def cpu_baseline(args, net, syn):
    """oracle/ (the CPU restatement: sequential voxeliser, hash rulebooks, gather-GEMM-scatter f32 — spconv's native CPU
    algorithm) timed on this host: (i) ONE thread, what a dataloader worker running spconv's CPU voxeliser + a CPU model
    would use; (ii) every core this job may use (physical cores, capped by sched_getaffinity and the cgroup's cpu.max), in
    the two forms a CPU deployment has: one scene per thread (scenes are independent; the conv kernel releases the GIL),
    and one scene at a time with OpenMP over the output tiles of each convolution — `value` is the
    faster of the two, both are reported.  Scenes are synthesised BEFORE the clocks start; each leg is bounded to ~10-20 s."""
    from concurrent.futures import ThreadPoolExecutor

    from oracle import oracle as O

    sd = {k: t.detach().cpu().numpy() for k, t in net.state_dict().items()}
    O.lib()
    model, phys, usable = host_cpu()
    threads = args.cpu_threads if args.cpu_threads > 0 else max(1, min(phys, usable))
    distinct = [syn.make_scene(s) for s in range(max(args.cpu_scenes, min(32, 2 * threads)))]

    def one(p):
        v, c, n = O.voxelize(p, syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, syn.MAX_POINTS_PER_VOXEL, syn.MAX_VOXELS_TEST)
        f = O.mean_vfe(v, n)
        idx = np.concatenate([np.zeros((c.shape[0], 1), np.int32), c], 1)
        O.backbone_forward(sd, f, idx, 1, net.sparse_shape)

    O.set_threads(1)
    one(distinct[0])                                       # warm-up (page faults, lazy loads)
    t0 = time.perf_counter()
    for p in distinct[:args.cpu_scenes]:
        one(p)
    t1 = time.perf_counter() - t0
    single = args.cpu_scenes / t1
    # (ii-a) one scene per thread: 2 scenes per thread (the distinct scenes cycled), ~2 / single seconds
    n_multi = 2 * threads
    scenes = [distinct[i % len(distinct)] for i in range(n_multi)]
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, scenes[:threads]))              # warm-up of the pool
        t0 = time.perf_counter()
        list(pool.map(one, scenes))
        tm = time.perf_counter() - t0
    multi = n_multi / tm
    # (ii-b) OpenMP over the output tiles of each convolution, scenes one after the other
    omp_threads = min(threads, int(O.lib().orc_max_threads()))
    O.set_threads(omp_threads)
    one(distinct[0])
    n_omp = max(2, min(len(distinct), int(10.0 * single * min(omp_threads, 8))))
    t0 = time.perf_counter()
    for p in distinct[:n_omp]:
        one(p)
    to = time.perf_counter() - t0
    O.set_threads(1)
    omp = n_omp / to
    return {"value": max(multi, omp), "unit": "scenes/s", "cores": threads, "kind": "port",
            "sample": f"the same synthetic scenes, batch 1, f32, voxelize + MeanVFE + VoxelResBackBone8x through oracle/ (sequential voxeliser, hash "
                      f"rulebook, gather-GEMM-scatter): {n_multi} scenes one per thread on {threads} threads in {tm:.1f} s = {multi:.2f} scenes/s; "
                      f"{n_omp} scenes with OpenMP over output tiles on {omp_threads} threads in {to:.1f} s = {omp:.2f} scenes/s; "
                      f"single-thread leg: {args.cpu_scenes} scenes in {t1:.1f} s",
            "scene_per_thread": {"value": multi, "threads": threads, "scenes": n_multi, "seconds": tm},
            "openmp_over_tiles": {"value": omp, "threads": omp_threads, "scenes": n_omp, "seconds": to},
            "single_thread": {"value": single, "cores": 1, "seconds": t1, "scenes": args.cpu_scenes},
            "host_cores": phys, "host_cores_usable": usable, "cpu_model": model}


def min_traffic_bytes(tag, n_out, b, tile_record_per_row=58):
    """what a launch of a TILED kernel has to move at least: features in and out once (+ residual), the tile rulebook, the weights"""
    cin, cout, K, res = tag[:4]
    return n_out * (cin * b + cout * b * (2 if res else 1) + tile_record_per_row) + K * cin * cout * b


STRIDED_CLASSES = {(16, 32, 27), (32, 64, 27), (64, 128, 27), (128, 128, 3)}   # the four SparseConv3d layers (spconv_backbone.py:205-234)


def rulebook_bytes_per_row(key, dtype):
    """bytes of rulebook a launch of this layer class reads per output row, in the format the engine gives it (DESIGN.md
    section 3): compact 32-byte records (stage 1 and 16 -> 32), 58-byte tile-rulebook rows (32 -> 32, 64 -> 64), the int32
    table (K x 4) for the class-sorted 128 -> 128 sweep and conv_out, nothing for the strided layers that resolve their
    neighbours inside the kernel; the f32 engine runs on tables throughout"""
    cin, cout, K = key
    if dtype != "bf16":
        return 4 * K
    if key in ((5, 16, 27), (16, 16, 27), (16, 32, 27)):
        return 32
    if key in ((32, 32, 27), (64, 64, 27)):
        return 58
    if key in ((32, 64, 27), (64, 128, 27)):
        return 0
    return 4 * K


def step_roofline(layers, n_points, n_voxels, b, dtype, ms_per_step, mfma_peak):
    """The whole step against the two PHYSICAL roofs.  layers: [(tag, P, n_out)] in execution order.
    min_traffic = what one step has to move through HBM if every tensor crossed it exactly once per use:
      voxeliser  N x 20 B points in, M x (16 B coords + 20 B means) out;
      per conv   n_in x Cin x b in + n_out x Cout x b out (+ n_out x Cout x b residual) + K x Cin x Cout x b weights
                 + its rulebook rows (rulebook_bytes_per_row) read once per launch and written once per rulebook;
      conv_input reads the f32 means (20 B per row), conv_out writes f32 (the boundary dtype).
    dense_equivalent_flops = sum over convs of 2 x n_out x K x Cin x Cout (what an output-stationary sweep multiplies,
    absent-neighbour zeros included); algorithmic_flops = sum of 2 x P x Cin x Cout (pairs that exist)."""
    byts = n_points * 20 + n_voxels * 36
    dense = alg = 0.0
    n_prev, seen_rb = n_voxels, set()
    for i, (tag, P, n) in enumerate(layers):
        cin, cout, K, res = tag[:4]
        key = (cin, cout, K)
        n_in = n_prev if key in STRIDED_CLASSES else n
        b_in = 4 if i == 0 else b
        b_out = 4 if i == len(layers) - 1 else b
        rb = rulebook_bytes_per_row(key, dtype)
        byts += n_in * cin * b_in + n * cout * b_out + (n * cout * b if res else 0) + K * cin * cout * b_in + n * rb
        rb_id = (key in STRIDED_CLASSES, n, rb)
        if rb_id not in seen_rb:            # (a rulebook is written once and shared by the layers of its indice_key)
            seen_rb.add(rb_id)
            byts += n * rb
        dense += 2.0 * n * K * cin * cout
        alg += 2.0 * P * cin * cout
        n_prev = n
    t = ms_per_step * 1e-3
    return {"min_traffic_bytes": float(byts), "hbm_GBps_min_traffic": byts / t / 1e9, "frac_hbm_min_traffic": byts / t / 1e9 / 8000.0,
            "dense_equivalent_flops": dense, "mfma_TFLOPs_dense_equivalent": dense / t / 1e12,
            "frac_mfma_dense_equivalent": dense / t / 1e12 / mfma_peak,
            "algorithmic_flops": alg, "mfma_TFLOPs_algorithmic": alg / t / 1e12, "ms_per_step": ms_per_step,
            "floor_ms": {"hbm": byts / 8e12 * 1e3, "mfma": dense / (mfma_peak * 1e12) * 1e3},
            "note": "physical roofs of the WHOLE step: minimum HBM traffic (every tensor once per use, rulebooks in the engine's formats) / "
                    "ms_per_step / 8 TB/s, and dense-equivalent matrix flops / ms_per_step / the dense MFMA peak of the dtype; `frac` above "
                    "stays SURVEY 8(d)'s gather-equivalent figure for the dominant kernel"}


def flat_summary(out):
    """FLAT top-level copies of the figures a reader of the one JSON line looks for first (the driver keeps the
    flat keys of the line and a short tail — round 5's nested `per_class`, `step`, `batch_sweep`, `pipelined`, `secondary` were
    cut).  Scalars only; every one of them is also where it was, nested."""
    f = {}

    def put(key, *path, scale=1.0):
        v = out
        for p in path:
            if not isinstance(v, dict) or p not in v:
                return
            v = v[p]
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            f[key] = float(v) * scale

    put("roofline_frac", "roofline", "frac")
    put("dominant_kernel_avg_launch_ms", "roofline", "avg_launch_ms")
    put("dominant_kernel_hbm_frac_from_traffic", "roofline", "hbm_frac_from_traffic")
    put("step_frac_hbm_min_traffic", "roofline", "step", "frac_hbm_min_traffic")
    put("step_frac_mfma_dense_equivalent", "roofline", "step", "frac_mfma_dense_equivalent")
    for cls in ("5x16k27", "16x16k27", "16x32k27", "32x32k27", "32x64k27", "64x64k27", "64x128k27", "128x128k27", "128x128k3"):
        put(f"ms_{cls}", "roofline", "per_class", cls, "ms_per_step")
        put(f"frac_gather_{cls}", "roofline", "per_class", cls, "frac_hbm_gather_equivalent")
        put(f"frac_mfma_{cls}", "roofline", "per_class", cls, "frac_mfma_dense_equivalent")
    put("cpu_baseline_scenes_per_s", "cpu_baseline", "value")
    for d in ("1_batch_in_flight", "2_batches_in_flight", "3_batches_in_flight"):
        put(f"pipelined_{d[0]}_scenes_per_s", "pipelined", d, "scenes_per_s")
    for b in ("1", "8", "64"):
        put(f"batch{b}_ms_per_step_graph", "batch_sweep", b, "ms_per_step_graph")
        put(f"batch{b}_scenes_per_s_graph", "batch_sweep", b, "scenes_per_s_graph")
        put(f"batch{b}_scenes_per_s_stream", "batch_sweep", b, "scenes_per_s_stream")
    put("batch1_scenes_per_s_2_in_flight", "batch_sweep", "1", "scenes_per_s_graph_2_in_flight")
    put("batch1_scenes_per_s_3_in_flight", "batch_sweep", "1", "scenes_per_s_graph_3_in_flight")
    put("fp32_engine_scenes_per_s", "secondary", "fp32_engine", "value")
    put("fp32_engine_roofline_frac", "secondary", "fp32_engine", "roofline", "frac")
    put("fp32_grade_engine_scenes_per_s", "secondary", "fp32_grade_engine", "value")
    put("box_seeker_scenes_per_s", "secondary", "box_seeker", "scenes_per_s")
    put("extraction_scenes_per_s", "secondary", "extraction", "scenes_per_s")
    put("extraction_ms_per_scene", "secondary", "extraction", "ms_per_scene_per_gpu")
    put("train_step_ms", "secondary", "train_step", "train_step_ms")
    put("train_step_cfg_ms", "secondary", "train_step_cfg", "train_step_ms")
    put("ten_sweep_scenes_per_s", "secondary", "ten_sweep", "scenes_per_s")
    put("first_bev_block_ms_bf16_rows", "secondary", "first_bev_block", "from_sparse_rows_ms", "bf16_rows")
    return f


def child_json(cmd, timeout):
    """last JSON line a child process prints (secondary measurements run in fresh processes: their own allocator history,
    hipGraph capture without this process's event-timed launches before it)"""
    import subprocess
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if not lines:
        raise RuntimeError((r.stderr or r.stdout)[-300:])
    return json.loads(lines[-1])


def measured_traffic(kname, B, dtype, budget_s=110.0):
    """HBM bytes per launch of kernel `kname`, MEASURED NOW: this script is run twice more as a child of rocprofv3 (3 steps each), once
    with --pmc FETCH_SIZE and once with --pmc WRITE_SIZE (separate passes, --kernel-trace only, as MI355X_MICROARCH.md prescribes),
    and the counters of the kernel's launches are averaged: (2 * FETCH_SIZE + WRITE_SIZE) * 1024 (KiB units; gfx950 FETCH_SIZE counts
    64 B per 128-B request).  -> (bytes, launches, note) or raises."""
    import shutil
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_traffic as PT
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        raise RuntimeError("rocprofv3 not found")
    vals = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="fnp_pmc_", dir="/tmp")
        cmd = [prof, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--batch", str(B), "--dtype", dtype, "--cpu-scenes", "0", "--no-sweep", "--no-secondary", "--no-traffic", "--steps", "3", "--warmup", "2",
               "--reps", "1"]
        p = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"),
                             start_new_session=True)
        try:
            p.wait(timeout=budget_s)
        except subprocess.TimeoutExpired:
            import signal
            os.killpg(p.pid, signal.SIGKILL)     # (the exact process group this call started)
            p.wait()
            shutil.rmtree(d, ignore_errors=True)
            raise RuntimeError(f"the {counter} pass did not finish in {budget_s:.0f} s")
        try:
            acc = PT.load(d, counter)
        finally:
            shutil.rmtree(d, ignore_errors=True)
        hit = [v for k, v in acc.items() if PT.short(k) == kname]
        if not hit:
            raise RuntimeError(f"no launch of {kname} in the {counter} pass")
        vals[counter] = hit[0]
    f, w = vals["FETCH_SIZE"], vals["WRITE_SIZE"]
    return (2.0 * sum(f) / len(f) + sum(w) / len(w)) * 1024.0, min(len(f), len(w))


DUMP_ROWS = 32768                 # rows kept per output tensor (every row when it has fewer)
DUMP_LIMIT_BYTES = 64 * 10 ** 6   # 128 scenes per step: ~52 MB


def dump_outputs(res, sparse_shape, out_dir):
    """--dump-outputs: the dict the timed path returned for its last batch, as out_dir/<name>.npy.  The voxeliser's outputs
    (voxel_coords [b, z, y, x], voxel_num_points, voxel_features) and, for each SparseConvTensor (x_conv1 .. x_conv4, out),
    <name>_features and <name>_indices; all float32 (bf16 features and int32 indices convert exactly), plus `counts` (float64,
    the site count of every stage).  The rows of a tensor are put in (b, z, y, x) order first, so that a build that emits them
    in another order compares equal, then at most DUMP_ROWS of them are kept at seeded positions: the same rows for the same
    row count, shared by the arrays of one tensor."""
    groups = [(res["voxel_coords"], sparse_shape, {k: res[k] for k in ("voxel_coords", "voxel_num_points", "voxel_features")})]
    for name in ("x_conv1", "x_conv2", "x_conv3", "x_conv4", "out"):
        t = res[name]
        groups.append((t.indices, t.spatial_shape, {f"{name}_features": t.features, f"{name}_indices": t.indices}))
    arrays = {"counts": np.asarray([int(c) for c in res["counts"]], np.float64)}
    for seed, (idx, shape, members) in enumerate(groups):
        i = idx.to(torch.int64)
        order = torch.argsort(((i[:, 0] * shape[0] + i[:, 1]) * shape[1] + i[:, 2]) * shape[2] + i[:, 3], stable=True)
        n = int(order.shape[0])
        if n > DUMP_ROWS:
            keep = np.sort(np.random.default_rng(seed).choice(n, DUMP_ROWS, replace=False))
            order = order[torch.from_numpy(keep).to(order.device)]
        for key, t in members.items():
            arrays[key] = t[order].float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"outputs to dump take {total} bytes"
    os.makedirs(out_dir, exist_ok=True)
    for key, a in arrays.items():
        np.save(os.path.join(out_dir, key + ".npy"), a)


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch N > 1 under torch.distributed.run "
                         f"(--nproc-per-node {args.gpus}); refusing to report a number for a different GPU count")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU path for the product)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1 or os.environ.get("FNP_BENCH_FORCE_DIST") == "1":   # (the switch: a one-rank process group, to rehearse the N > 1 path on one GPU)
        import torch.distributed as dist_

        dist = dist_
        dist.init_process_group("nccl", device_id=dev)

    from findnpropagate_amd import lib, sparse as S, synthetic as syn
    from findnpropagate_amd.backbones_3d import VoxelResBackBone8x

    lib.load()
    B = args.batch
    grid = np.round((np.array(syn.POINT_CLOUD_RANGE[3:]) - np.array(syn.POINT_CLOUD_RANGE[:3])) / np.array(syn.VOXEL_SIZE)).astype(int)
    net = syn.init_backbone_weights(VoxelResBackBone8x({"USE_BIAS": False, "FNP_DTYPE": args.dtype}, 5, grid), seed=0)
    net = net.to(dev).eval()
    seeds = [rank * B + i for i in range(B)]
    pts_np, off_np = syn.make_batch(seeds)
    pts = torch.from_numpy(pts_np).to(dev)
    off = torch.from_numpy(off_np).to(dev)
    cfg = S.make_voxel_cfg(syn.VOXEL_SIZE, syn.POINT_CLOUD_RANGE, 5, syn.MAX_POINTS_PER_VOXEL, syn.MAX_VOXELS_TEST)
    eng = net.engine()

    probe_graphs = [False]   # the timed step replays the two-graph capture (decided below, once the dominant class is known)
    pipe_box = [None]        # --launch pipeline: the PointsPipeline of the timed region (built below, once the dominant class is known)

    def step():
        with torch.no_grad():
            if args.graph and eng.rulebook_log is None and eng.profile is None:
                return net.forward_points_graphed(pts, off, B, cfg)
            if probe_graphs[0] and eng.rulebook_log is None:
                return net.forward_points_graphed(pts, off, B, cfg, probe=True)
            return net.forward_points(pts, off, B, cfg)  # ends with the one host sync that sizes the outputs

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        res = step()
    # rulebook statistics for the roofline (outside the timed region)
    eng.rulebook_log = []
    res = step()
    rb_log, eng.rulebook_log = eng.rulebook_log, None
    counts = res["counts"]
    stats = {}
    layers_in_order = []
    for tag, rb, n_dev in rb_log:
        n = int(n_dev.item())
        key = id(rb.nbr)
        if key not in stats:
            stats[key] = int((rb.nbr[:, :n] >= 0).sum().item())
        stats.setdefault(("tags", tag), []).append((stats[key], n))
        layers_in_order.append((tag, stats[key], n))
    torch.cuda.synchronize()

    # Which layer class dominates, and the per-class times quoted beside the roofline, come from a few
    # UNTIMED steps with every conv launch bracketed by events; in the timed region only the dominant class
    # is bracketed (an event pair per launch is a queue marker: 42 of them per step cost ~4 % of the step).
    per_class_ms = None
    if not args.no_events and not args.graph:
        probe_steps = 5
        per_step = []
        for _ in range(probe_steps):
            eng.profile = []
            step()
            torch.cuda.synchronize()
            acc = {}
            for tag, e0, e1 in eng.profile:
                acc[tag[:3]] = acc.get(tag[:3], 0.0) + e0.elapsed_time(e1)
            per_step.append(acc)
        # (median over the probe steps: an allocator growth or a first-launch attribute call inside a bracket
        # would otherwise be booked on that class)
        per_class_ms = {k: float(np.median([a[k] for a in per_step])) for k in per_step[0]}
        # dominant class = largest time per step; classes within 15 % of it are a tie (two of them trade places
        # from run to run), broken towards the lower achieved rate so that the quoted fraction is never the
        # flattering one
        top = max(per_class_ms.values())
        def rate(k):
            tags = [t for t in stats if isinstance(t, tuple) and t[0] == "tags" and t[1][:3] == k]
            byts = sum(algorithmic_bytes(t[1], P, n, 2 if args.dtype == "bf16" else 4) for t in tags for (P, n) in stats[t])
            return byts / per_class_ms[k]
        tied = [k for k, v in per_class_ms.items() if v >= 0.85 * top]
        eng.profile_only = {min(tied, key=rate)}
        eng.profile = []
        # The timed step: when the dominant class is the last SubM stage's (128 -> 128, 3x3x3: the engine can leave exactly those
        # launches out of its captured graphs), the step is replayed from two hipGraphs with those four launches in between as
        # plain launches, each between two timing events — the replayed step's throughput AND the dominant kernel's duration
        # measured inside the same timed region.  Otherwise (or --launch stream) every kernel is a plain launch as before.
        if args.launch in ("graphs", "pipeline") and eng.profile_only == {(128, 128, 27)}:
            probe_graphs[0] = True
            try:
                for _ in range(2):   # (capture + one replay, untimed)
                    step()
                torch.cuda.synchronize()
            except Exception as e:   # (a capture that cannot be taken here must not cost the run its headline: plain launches then)
                print(f"bench: two-graph step unavailable ({repr(e)[:200]}); timing plain stream launches", file=sys.stderr)
                probe_graphs[0] = False
                torch.cuda.synchronize()
                step()
                torch.cuda.synchronize()
            eng.profile = []
        if args.launch == "pipeline" and probe_graphs[0] and args.in_flight > 1:
            # THE BATCH PATH (round 6): --in-flight batches in flight.  Every slot of the pipeline owns an engine, a stream and the
            # same two-graph capture as above; a step = take the oldest batch's outputs if the pipeline is full, submit the next
            # batch; the region ends with the pipeline drained, so exactly --steps batches go in AND come out between the barriers.
            try:
                with torch.no_grad():
                    pipe = net.points_pipeline(B, cfg, depth=args.in_flight, capacity=(pts.shape[0] + 65535) // 65536 * 65536, probe=True)
                    for r_p in pipe.map([(pts, off)] * (2 * args.in_flight + args.warmup)):
                        pass
                    torch.cuda.synchronize()
                    assert [int(c) for c in r_p["counts"]] == [int(c) for c in counts], "pipelined step: other site counts than the eager step"
                pipe_box[0] = pipe
            except Exception as e:
                print(f"bench: pipelined step unavailable ({repr(e)[:200]}); timing one batch at a time", file=sys.stderr)
                pipe_box[0] = None
                torch.cuda.synchronize()
    # The timed region (EXACTLY --steps steps between two barrier + synchronize pairs, MAX over ranks) is repeated --reps
    # times back to back; `value` / `ms_per_step` are those of the MEDIAN repetition and the whole list is reported (one
    # 0.12 s region is a single draw: boxes of the pool differ by +-8 %, and so do repetitions on one box by 1-2 %).
    rep_elapsed, rep_prof = [], []
    pipe = pipe_box[0]
    for _ in range(max(1, args.reps)):
        if eng.profile is not None:
            eng.profile = []
        if pipe is not None:
            pipe.profile = []
        barrier()
        t0 = time.perf_counter()
        if pipe is not None:
            with torch.no_grad():
                for _ in range(args.steps):
                    if len(pipe.pending) == pipe.depth:
                        res = pipe.result()
                    pipe.submit(pts, off)
                while pipe.pending:          # (every step's outputs are produced and taken inside the region)
                    res = pipe.result()
        else:
            for _ in range(args.steps):
                res = step()
        barrier()
        t1 = time.perf_counter()
        e = t1 - t0
        if dist is not None:
            t = torch.tensor([e], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e = float(t.item())
        rep_elapsed.append(e)
        rep_prof.append(pipe.profile if pipe is not None else eng.profile)
    order = sorted(range(len(rep_elapsed)), key=lambda i: rep_elapsed[i])
    mid = order[(len(order) - 1) // 2]
    elapsed = rep_elapsed[mid]
    prof = rep_prof[mid]
    eng.profile, eng.profile_only = None, None
    if pipe is not None:
        pipe.profile = None
    counts = res["counts"]          # (of the last timed step)
    if rank == 0 and args.dump_outputs:
        dump_outputs(res, net.sparse_shape, args.dump_outputs)

    # Per-rank shard evidence: every rank's stage counts and a checksum of its voxel coordinates travel to
    # rank 0 in ONE all_gather after the timed region, so that a multi-GPU run can be checked for N DISTINCT shards (rank r takes
    # seeds r*B .. r*B + B - 1) from its single JSON line.  Not a data-path collective: the step itself exchanges nothing.
    vc = res["voxel_coords"].to(torch.int64)
    lin = ((vc[:, 0] * 41 + vc[:, 1]) * 1440 + vc[:, 2]) * 1440 + vc[:, 3]
    mine = torch.tensor([int(c) for c in counts] + [int((lin * 1000003 % 2147483647).sum().item()), seeds[0], seeds[-1]], dtype=torch.int64, device=dev)
    if dist is not None:
        allr = torch.empty((world * mine.numel(),), dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(allr, mine)
        allr = allr.view(world, -1).tolist()
    else:
        allr = [mine.tolist()]
    per_rank = [{"rank": r, "seeds": [row[6], row[7]], "site_counts": row[:5], "voxel_coords_checksum": row[5]} for r, row in enumerate(allr)]

    out = {
        "metric": "NuScenes scenes/s (30k pts, Transfusion voxel backbone)",
        "value": world * B * args.steps / elapsed,
        "unit": "scenes/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "repetitions": {"count": len(rep_elapsed), "steps_each": args.steps, "reported": "median",
                        "scenes_per_s": [world * B * args.steps / e for e in rep_elapsed]},
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": "synthetic",
        "config": {"workload": "synthetic 30k-point nuScenes-like scenes: voxelize + MeanVFE + VoxelResBackBone8x "
                               "(BASELINE.json configs[1])",
                   "scenes_per_step_per_gpu": B, "points_per_scene": int(pts_np.shape[0] // B),
                   "voxels_per_scene": int(counts[0] // B), "sparse_shape": [41, 1440, 1440],
                   "site_counts": [int(c) for c in counts], "weights": "seeded random init",
                   "per_rank": per_rank, "shards_distinct": len({r["voxel_coords_checksum"] for r in per_rank}) == world,
                   "parallelism": f"scenes sharded {world}x, no data-path collective",
                   # the statistic the tile-rulebook kernels are gated on (share of 32-row groups with an escape entry, stages 2 / 3;
                   # above 0.004 a stage runs on the gather kernels) and which stages that switched off in this run
                   "tile_gate": {"escape_share": {f"stage{li + 2}": round(v, 6) for li, v in sorted(eng.tile_escape_share.items())},
                                 "stages_on_gather_kernels": [li + 2 for li in eng._heur_key()]},
                   "launch": ("hipGraph replay" if args.graph else
                              f"{pipe.depth} batches in flight (the batch path's default, forward_points_iter): per batch two hipGraphs on the "
                              "slot's stream with the dominant kernel's four launches stream-launched between them and bracketed with HIP "
                              "events; a step = take the oldest batch's outputs, submit the next; the region ends drained" if pipe is not None else
                              "two hipGraphs per step (index chain on a second branch) with the dominant kernel's four launches "
                              "stream-launched between them and bracketed with HIP events" if probe_graphs[0] else "stream launches"),
                   "batches_in_flight": pipe.depth if pipe is not None else 1},
    }

    if rank == 0 and prof:
        b = 2 if args.dtype == "bf16" else 4
        per = {}
        for tag, e0, e1 in prof:
            per.setdefault(tag[:3], []).append((e0.elapsed_time(e1), tag))
        # dominant layer class = largest total time; one class = one kernel name (template instance)
        cls = max(per, key=lambda k: sum(x[0] for x in per[k]))
        ms = [x[0] for x in per[cls]]
        byts = []
        for _, tag in per[cls]:
            P, n = stats[("tags", tag)][0]
            byts.append(algorithmic_bytes(tag, P, n, b))
        avg_ms = float(np.mean(ms))
        avg_bytes = float(np.mean(byts))
        achieved = avg_bytes / (avg_ms * 1e-3) / 1e9
        cin, cout, K = cls
        flops = 2.0 * float(np.mean([stats[("tags", tag)][0][0] for _, tag in per[cls]])) * cin * cout
        dense_flops = 2.0 * float(np.mean([stats[("tags", tag)][0][1] for _, tag in per[cls]])) * K * cin * cout
        win = "true" if (per[cls][0][1][4] and K == 27 and (cin, cout) == (64, 64)) else "false"
        mb = 3 if cout >= 128 else 2 if (cin, cout) in ((16, 16), (16, 32), (32, 32), (64, 64)) else 4   # launch_mfma_k
        mb32 = 4 if cout <= 64 else 3                                                                    # launch_f32
        srt = ",sorted" if (args.dtype == "bf16" and K == 27 and S.sorted_by_default(cin, cout, torch.bfloat16, int(pts.shape[0] * eng.cap_factor[2]))) else ""
        kname = (f"spconv_mfma_kernel<{cin},{cout},{mb},{K if K == 27 else 0},{win},bf16{srt}>"
                 if args.dtype == "bf16" else f"spconv_mfma_f32_kernel<{cin},{cout},{mb32}>")
        # HBM bytes per launch of that kernel: MEASURED in a --full run (measured_traffic: PMC counters need rocprofv3 around a
        # process, so this script is started twice more, 3 steps each, as a child of rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE; gfx950
        # FETCH_SIZE x2 correction applied).  Plain runs, child runs (--no-secondary, --no-traffic) and a failed measurement quote the
        # committed passes of the same command (profiles/r0N_pmc_traffic_<dtype>_b<B>.json); null when there is neither
        traffic, traffic_src = None, None
        if rank == 0 and world == 1 and args.full and not args.no_traffic and not args.no_secondary and not args.graph:
            try:
                traffic, n_l = measured_traffic(kname, B, args.dtype)
                traffic_src = (f"measured in this run: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; --kernel-trace only) of `bench.py --batch {B} --steps 3` "
                               f"as child processes, {n_l} launches of the kernel averaged, (2*FETCH_SIZE + WRITE_SIZE)*1024")
            except Exception as e:
                traffic, traffic_src = None, "live PMC passes failed (" + repr(e)[:160] + "); "
        for name in (() if traffic else (f"r06_pmc_traffic_{args.dtype}_b{B}.json", f"r05_pmc_traffic_{args.dtype}_b{B}.json", f"r04_pmc_traffic_{args.dtype}_b{B}.json", f"r03_pmc_traffic_{args.dtype}_b{B}.json", f"r02_pmc_traffic_{args.dtype}_b{B}.json",
                     f"r01_pmc_traffic_b{B}.json" if args.dtype == "bf16" else "")):
            try:
                pj = json.load(open(os.path.join(ROOT, "profiles", name)))
                if pj.get("batch") == B and kname in pj["kernels"]:
                    traffic, traffic_src = pj["kernels"][kname]["hbm_bytes_corrected"], (traffic_src or "") + f"profiles/{name} (committed rocprofv3 --pmc passes of this command; not measured in this run)"
                    break
            except Exception:
                continue
        # every conv class of the step against ITS roofs (medians of the bracketed probe steps): SURVEY 8(d) gather-equivalent
        # bytes (an upper bound on useful traffic, NOT a roof for the tiled kernels, where a row enters LDS once per tile:
        # those are quoted against their minimum traffic), and the matrix pipe in dense-equivalent flops (the absent-
        # neighbour zeros an output-stationary sweep multiplies included) against the dense peak of the dtype
        mfma_peak = 2500.0 if args.dtype == "bf16" else 157.3
        table = {}
        for key, ms_step in (per_class_ms or {}).items():
            tags = [t[1] for t in stats if isinstance(t, tuple) and t[0] == "tags" and t[1][:3] == key]
            items = [(tag, P, n) for tag in tags for (P, n) in stats[("tags", tag)]]
            if not items:
                continue
            ci, co, kk = key
            alg = sum(algorithmic_bytes(tag, P, n, b) for tag, P, n in items)
            fl_alg = sum(2.0 * P * ci * co for _, P, _ in items)
            fl_dense = sum(2.0 * n * kk * ci * co for _, _, n in items)
            row = {"launches_per_step": len(items), "ms_per_step": ms_step,
                   "gather_equivalent_GBps": alg / ms_step / 1e6, "frac_hbm_gather_equivalent": alg / ms_step / 1e6 / 8000.0,
                   "mfma_TFLOPs_algorithmic": fl_alg / ms_step / 1e9, "mfma_TFLOPs_dense_equivalent": fl_dense / ms_step / 1e9,
                   "frac_mfma_dense_equivalent": fl_dense / ms_step / 1e9 / mfma_peak}
            if args.dtype == "bf16" and kk == 27 and ci == co and ci in S.TILED_CHANNELS and all(tag[4] for tag, _, _ in items):
                mt = sum(min_traffic_bytes(tag, n, b) for tag, _, n in items)
                row.update({"kernel": f"spconv_tile{ci}_kernel", "min_traffic_GBps": mt / ms_step / 1e6, "frac_hbm_min_traffic": mt / ms_step / 1e6 / 8000.0,
                            "note": "tiled kernel: gather-equivalent bytes exceed what it moves; min traffic = rows in/out once + residual + tile rulebook + weights"})
            table[f"{ci}x{co}k{kk}"] = row
        common = {
            "traffic": traffic, "traffic_source": traffic_src,
            "hbm_frac_from_traffic": (traffic / (avg_ms * 1e-3) / 1e9 / 8000.0) if traffic else None,
            "kernel": kname,
            "avg_launch_ms": avg_ms, "launches_timed": len(ms), "algorithmic_bytes_per_launch": avg_bytes,
            "algorithmic_flops_per_launch": flops, "dense_equivalent_flops_per_launch": dense_flops,
            "time_share_of_step": sum(ms) / (1e3 * elapsed),
            "all_conv_classes_ms_per_step": {f"{k[0]}x{k[1]}k{k[2]}": v for k, v in (per_class_ms or {}).items()},
            "all_conv_classes_note": "median of 5 untimed steps with every conv launch bracketed; the timed region brackets the dominant class only",
            "per_class": table,
        }
        tflops = flops / (avg_ms * 1e-3) / 1e12
        if args.dtype == "bf16":
            # `achieved` = SURVEY 8(d) algorithmic (gather-equivalent) bytes / launch time: most of those bytes are served by L2 / MALL
            # (`traffic` is what reaches HBM), so `frac` says how fast the gather path runs in HBM-peak units, not HBM utilisation
            out["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                               "mfma_tflops_algorithmic": tflops, "mfma_frac_dense_equivalent": dense_flops / (avg_ms * 1e-3) / 1e12 / 2500.0, **common}
        else:
            # f32 runs on v_mfma_f32_16x16x4_f32 at the f32 vector rate (157.3 TFLOP/s dense): that pipe, not memory, bounds it
            out["roofline"] = {"bound": "mfma", "achieved": tflops, "peak": 157.3, "unit": "TFLOP/s", "frac": tflops / 157.3,
                               "hbm_gbs_algorithmic": achieved, **common}
        out["roofline"]["step"] = step_roofline(layers_in_order, int(pts.shape[0]), int(counts[0]), b, args.dtype,
                                                1e3 * elapsed / args.steps, mfma_peak)

    if rank == 0 and world == 1 and args.full and not args.no_sweep and not args.graph:
        # Extra fields (the headline stays `value` at --batch): the same path at 1 and 8 scenes per step — batch size 1 is
        # what the reference's extraction script and configs[0] run — as stream launches and replayed from a hipGraph, both
        # measured HERE, in this process, after the event-timed launches above (round 2 had to move the graph leg into a
        # child process: a replay after eager forwards faulted.  Cause, fixed in round 3: the voxeliser's captured
        # hipMemsetAsync replayed with the fill value of a later eager memset — DESIGN.md section 2).
        sweep = {}
        for b in (1, 8, 64):
            if b == B:
                continue
            p_np, o_np = syn.make_batch(list(range(b)))
            p_b, o_b = torch.from_numpy(p_np).to(dev), torch.from_numpy(o_np).to(dev)
            row = {}
            with torch.no_grad():
                for mode, fwd in (("stream", net.forward_points), ("graph", net.forward_points_graphed)):
                    try:
                        for _ in range(5):
                            fwd(p_b, o_b, b, cfg)
                        dts = []
                        for _ in range(3):   # (three regions of 20 steps, the median: one hiccup inside a single region was the number before)
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            for _ in range(20):
                                r_b = fwd(p_b, o_b, b, cfg)
                            torch.cuda.synchronize()
                            dts.append((time.perf_counter() - t0) / 20)
                        dt = sorted(dts)[1]
                        row[f"ms_per_step_{mode}"], row[f"scenes_per_s_{mode}"] = 1e3 * dt, b / dt
                        row[f"site_counts_{mode}"] = [int(c) for c in r_b["counts"]]
                    except Exception as e:   # the extra field is best effort: never lose the headline over it
                        row[f"{mode}_error"] = repr(e)[:200]
            row["graph_equals_stream"] = row.get("site_counts_graph") == row.get("site_counts_stream")
            if b == 1:
                # frames that arrive one at a time, 2 / 3 of them in flight (PointsPipeline: a hipGraph, an engine and a stream
                # per slot): the frame RATE of a one-scene stream; the latency of a frame is ms_per_step_graph
                for depth in (2, 3):
                    try:
                        with torch.no_grad():
                            pipe = net.points_pipeline(1, cfg, depth=depth, capacity=65536)
                            frames = [(p_b, o_b)] * 60
                            for r_p in pipe.map(frames[:10]):
                                pass
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            for r_p in pipe.map(frames):
                                pass
                            torch.cuda.synchronize()
                            dt = (time.perf_counter() - t0) / len(frames)
                        row[f"scenes_per_s_graph_{depth}_in_flight"] = 1.0 / dt
                        row[f"pipeline_{depth}_equals_stream"] = [int(c) for c in r_p["counts"]] == row.get("site_counts_stream")
                        del pipe
                    except Exception as e:
                        row[f"pipeline_{depth}_error"] = repr(e)[:200]
            sweep[str(b)] = row
        out["batch_sweep"] = sweep
        # like-for-like with rounds 1-3 (the default went from 64 to 128 scenes per step in round 4): the same replayed
        # step at 64 scenes per step, beside `value`
        if B == 64:
            out["value_at_64"] = out["value"]
        elif "scenes_per_s_graph" in sweep.get("64", {}):
            out["value_at_64"] = sweep["64"]["scenes_per_s_graph"]
        # The same 64-scene step with several BATCHES in flight (PointsPipeline: a hipGraph, an engine and a HIP stream per slot;
        # results identical per batch): what a server that is handed batches back to back gets out of the card — the latency-bound
        # index kernels of one batch run under the convolutions of another.  Reported beside `value`, which stays one batch at a time.
        # With ONE batch in flight this is the one-graph replay of the same step (the engine captures its index chain — rank
        # grids, rulebooks, class sort: coordinates only — on a second branch that runs beside the convolutions of the stage
        # before); `value`'s step is the same thing cut into two graphs around the dominant kernel's launches.
        try:
            pl = {}
            with torch.no_grad():
                cap = (pts.shape[0] + 65535) // 65536 * 65536
                for depth in (1, 2, 3):   # (1: the plain hipGraph replay of the step — its index chain runs on a second branch)
                    pipe = net.points_pipeline(B, cfg, depth=depth, capacity=cap)
                    frames = [(pts, off)] * 20
                    for r_p in pipe.map(frames[:2 * depth]):
                        pass
                    dts = []
                    for _ in range(3):   # (three passes of 20 batches, the median: one 0.1 s pass is a single draw)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for r_p in pipe.map(frames):
                            pass
                        torch.cuda.synchronize()
                        dts.append((time.perf_counter() - t0) / len(frames))
                    dt = sorted(dts)[1]
                    pl[f"{depth}_batch{'es' if depth > 1 else ''}_in_flight"] = {"scenes_per_s": B / dt, "ms_per_step": 1e3 * dt,
                                                        "site_counts_equal_value_run": [int(c) for c in r_p["counts"]] == [int(c) for c in counts]}
                    del pipe
            out["pipelined"] = pl
        except Exception as e:
            out["pipelined"] = {"error": repr(e)[:200]}

    if rank == 0 and world == 1 and args.full and not args.no_secondary and not args.graph and args.dtype == "bf16":
        # SURVEY 8(d)'s secondary metrics, each from a fresh child process (best effort: never lose the headline over one)
        py, T = sys.executable, os.path.join(ROOT, "tools")
        sec = {}
        # the headline is safe before any child starts: one line on stderr (stdout keeps its ONE line, printed at the end)
        print("bench: headline before the secondary measurements: " + json.dumps({k: out[k] for k in ("metric", "value", "unit", "ms_per_step")}),
              file=sys.stderr, flush=True)
        t_budget = time.perf_counter() + args.secondary_budget     # one wall-clock budget for all of them
        jobs = {
            "fp32_engine": ([py, os.path.abspath(__file__), "--batch", "64", "--dtype", "fp32", "--no-sweep", "--no-secondary", "--cpu-scenes", "0",
                             "--steps", "5", "--warmup", "2", "--reps", "3"], 240),
            "box_seeker": ([py, os.path.join(T, "bench_seeker.py"), "--batch", "64", "--cpu-scenes", "0"], 180),
            "extraction": ([py, os.path.join(T, "bench_extract.py"), "--scenes", "256", "--force-collective"], 240),
            "train_step": ([py, os.path.join(T, "bench_train.py"), "--batch", "16"], 240),
            # the step transfusion_lidar.yaml actually runs per GPU (BATCH_SIZE_PER_GPU 4, :147; MAX_SWEEPS 10, nuscenes_dataset.yaml:5; AMP,
            # train_utils.py:135-176): four 10-sweep scenes under autocast(fp16) + GradScaler + clip_grad_norm_
            "train_step_cfg": ([py, os.path.join(T, "bench_train.py"), "--batch", "4", "--sweeps", "10", "--amp", "--reps", "6"], 240),
            "first_bev_block": ([py, os.path.join(T, "bench_bev.py"), "--batch", "16"], 240),
            # the density transfusion_lidar.yaml feeds the backbone (nuscenes_dataset.yaml:5 MAX_SWEEPS 10): emulated 10-sweep scenes
            "ten_sweep": ([py, os.path.join(T, "bench_sweeps.py"), "--batch", "8"], 240),
            # the f32 result on the BF16 matrix pipe (FNP_DTYPE: bf16x3), with its measured deviation from the f32 engine
            "fp32_grade_engine": ([py, os.path.join(T, "bench_x3.py"), "--batch", "64"], 240),
        }
        for name, (cmd, to) in jobs.items():
            left = t_budget - time.perf_counter()
            if left < 20:
                sec[name] = {"skipped": f"the shared budget of {args.secondary_budget:.0f} s for secondary measurements was spent"}
                continue
            try:
                j = child_json(cmd, min(to, left))
                if name == "fp32_engine":
                    j = {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "scenes_per_step": 64,
                         "repetitions": j.get("repetitions"), "note": "FNP_DTYPE fp32: v_mfma_f32_16x16x4_f32, bit-identical to the CPU oracle (the 1e-4 mode)",
                         "roofline": {k: j["roofline"][k] for k in ("bound", "achieved", "peak", "unit", "frac", "kernel", "avg_launch_ms",
                                                                    "time_share_of_step", "algorithmic_flops_per_launch") if k in j.get("roofline", {})}}
                sec[name] = j
            except Exception as e:
                sec[name] = {"error": repr(e)[:300]}
        out["secondary"] = sec

    if rank == 0 and world == 1 and args.full and args.cpu_scenes > 0:   # (baseline leg: N = 1 only)
        out["cpu_baseline"] = cpu_baseline(args, net, syn)
    if rank == 0:
        out.update(flat_summary(out))
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
