#!/usr/bin/env python3
"""bench.py — Mray/s of the jade path-tracing hot path on MI355X.

Contract (driver): python bench.py --gpus N --steps K --warmup W ; for N > 1 the driver launches it with
torch.distributed.run, one rank per GPU (RCCL).  Started by hand with --gpus N > 1 and no launcher, it starts
that launcher itself as a child process — before anything touches the GPU — and exits with its code.  One JSON
line on rank 0.

Workload (BASELINE.json configs[2]/[3]): the 70k-triangle jade statue scene at 1920x1080.  A "step" is one pass of
the hot path adding `spp_per_step` samples to every pixel this rank owns; the per-sample RNG streams and radiance
sums stay on the GPU between steps, so K steps are K*spp_per_step samples of the same render, not K restarts; the
defaults (4 steps x 1024 spp) are exactly the 4096-spp render BASELINE.json names.  Multi-GPU: the image's 16x16
tiles are dealt (tx + ty) % N to the ranks and the samples per step scale with N, so per-GPU work per step is
constant ("weak"); after the timed steps the framebuffer is collected with ONE gather (RCCL; through host memory over gloo if
RCCL cannot be brought up on some rank - `exchange` says which), timed separately as gather_ms.  The barriers around the timed
region and the reduction of the ranks' counts run over gloo: the whole-job figure does not depend on RCCL's bootstrap.  A step may hand its last few unfinished paths to the next step (jade_render_flush, jade_rt.h); the
warm-up is flushed before the clock starts and the K timed steps are flushed before it stops, so every sample of
the K steps — `samples` = K * spp * pixels, and all their rays — is computed inside the timed region.

A plain run sets up, warms up, times the K steps, writes their outputs with --dump-outputs DIR (dump_outputs) and prints
the line.  --full adds, after the timed steps, what the headline figure does not need: the side runs with the other walks,
parity_check, cpu_baseline and the extras below (N = 1 only).

value = (primary + secondary rays traced by all ranks in the K timed steps) / max-over-ranks wall time, Mray/s.
        A ray = one hitBVH query (PathTrace.cu:795).
rooflines: the dominant kernel, k_trace (BVH traversal + triangle tests), against the three resources a traversal without
        matrix work can be bound by.  Each: achieved = (per-ray counter figure from the rocprofv3 --pmc passes of this same
        command, profiles/k_trace_counters.json) x (rays this run traced) / (k_trace time of this run, HIP events on the
        kernel's own stream).
          valu  VALU lane-operations (SQ_THREAD_CYCLES_VALU) against 1024 SIMDs x 32 lanes/clock x 2.4 GHz;
          l2    requests to the XCDs' L2s (TCC_HIT + TCC_MISS) x 64 B against the 16.8 TB/s MI355X_MICROARCH.md measures for
                gathers served by the L2 (its low end: 16.8-18.8);
          hbm   fabric-side bytes (FETCH_SIZE x the factor tools/fetch_calib measured for this access pattern + WRITE_SIZE)
                against 8 TB/s.
        `roofline` is the one with the largest fraction - the binding resource - and `binding` names it.  The per-ray
        figures belong to a build: profiles/k_trace_counters.json carries a hash of csrc/ and the fractions are null when
        the tree's differs (a kernel edit without re-profiling must not keep the old numbers).
        `algorithmic`: SURVEY.md 8d's 40 B per node record + 36 B per triangle test, per kernel (V and T are counted
        separately for k_light and k_trace; k_trace's V and T are the reference walk's side run's under --full, the timed
        walk's own without it); it exceeds the HBM peak when the scene is cache-resident, which is why it is reported beside
        the rooflines and not as one.
parity_check: the frame this run rendered (every sample of warm-up + timed steps) against the oracle on a few of its
        16x16 tiles - statue, mirror floor, sky - at the full sample count: relative L2 of the radiance, largest BGR8
        difference.  Outside the timed region; part of the cpu_baseline leg (the oracle is the checker, never the product).
cpu_baseline: the CPU oracle ("port": the reference has no CPU integrator) on a bounded sample of the same scene,
        rank 0 at N = 1 only.
extras (N = 1): secondary rays by call site, and the same scene with the camera moved in until the statue fills
        the frame (every pixel a jade path): the throughput on the rays the headline frame has few of.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0                      # MI355X_MICROARCH.md: HBM3E 8 TB/s
L2_GATHER_PEAK_GBS = 16800.0               # MI355X_MICROARCH.md, "Indexed rows": rows served by the XCDs' L2s, 16.8-18.8 TB/s chip-wide
# VALU issue roof (MI355X_MICROARCH.md: 4 SIMD-32 per CU, a wave64 VALU instruction issues in 2 clocks): 32 lane-operations per
# clock per SIMD.  That rate needs instructions the sequencer can pair (SQ_ACTIVE_INST_VALU2); a wave's own dependent stream issues
# one per 4 clocks, which is the unit SQ_ACTIVE_INST_VALU counts in (1.007 quad-cycles per VALU instruction in every kernel
# here).  The first k_trace of round 2 sat at 4 x ACTIVE_INST_VALU / SIMD-cycles = 1.05 of a possible 2 and its time followed
# its instruction count; the final one issues a third fewer instructions and sits at 0.7.  The roofline below
# is priced against the full 2-clock rate, `issue_busy_of_2` says how far the issue side is from it.
VALU_PEAK_TLANEOPS = 1024 * 32 * 2.4e9 / 1e12  # 256 CUs x 4 SIMDs x 32 lanes, 2.4 GHz = 78.6 T lane-ops/s
# The issue roof of the instruction kinds k_trace is made of (min / max, compare, select, integer, packed fp32): ONE wave64 instruction
# per SIMD per 4 clocks at any occupancy - measured, profiles/valu_calibration.json (tools/calib/valu_calib.hip); only unpacked fp32
# add / mul / fma and v_mov_b32 issue at up to one per 2 clocks, which is what the lane-operation peak above assumes of every instruction
VALU_ISSUE_PEAK_GINST = 1024 * 0.25 * 2.4e9 / 1e9  # 614 G wave-instructions/s


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--spp-per-step", type=int, default=1024, help="samples per pixel per step at N = 1")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the statue-filling camera variant")
    ap.add_argument("--bvh", default="sah", choices=["sah", "lbvh", "ploc"],
                    help="sah: the reference's host builder (default, what the metric is quoted on); lbvh / ploc: GPU builders")
    ap.add_argument("--bvh-leaf", type=int, default=0, help="triangles per leaf for the GPU builders (0: 8 for lbvh as in the reference, 3 for ploc)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl (= RCCL) for real runs; gloo rehearses the multi-rank flow with every rank on one GPU")
    ap.add_argument("--virtual-rank", type=int, default=0, help="with --virtual-ranks: which rank's share of the tiles (default 0)")
    ap.add_argument("--virtual-ranks", type=int, default=0,
                    help="development: render rank 0's share of a V-GPU run on this one GPU (partition and spp as at N=V)")
    ap.add_argument("--cpu-spp", type=int, default=8, help="oracle sample: spp over the full frame")
    ap.add_argument("--max-state-gb", type=float, default=0.0, help="jade_render_params.max_state_bytes: device memory for path records + partial sums (0 = the default, 60 %% of what is free)")
    ap.add_argument("--no-parity-check", action="store_true", help="skip the oracle spot check of the rendered frame")
    ap.add_argument("--walk", default=None, choices=["reference", "early_exit", "cached"],
                    help="jade_render_params.walk in the timed region.  early_exit (the default): JADE_WALK_EARLY_EXIT; cached: "
                         "JADE_WALK_EARLY_EXIT_CACHED - early exits, and yes/no queries first look where earlier ones found their answer (the same "
                         "frame bit for bit; measured slower on C3, DESIGN.md 3.3d); reference: every query walks what the reference walks")
    ap.add_argument("--side-steps", type=int, default=0, help="steps of the side runs with the other walks (0 = as many as --steps, with --warmup warm-up steps)")
    ap.add_argument("--reference-walk", action="store_true",
                    help="jade_render_params.walk = JADE_WALK_REFERENCE in the timed region: every query walks what the reference walks "
                         "(the default, JADE_WALK_EARLY_EXIT, ends shadow / environment-visibility walks at the hit that settles them: the same frame, bit for bit)")
    ap.add_argument("--parity-rays", type=float, default=1.2e8, help="oracle rays the parity check may cost (about 7 Mray/s on 16 cores)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: the side runs with the other walks, the close-up and "
                         "glass-statue variants, the CPU baseline and the oracle parity check (--no-extras / --no-cpu-baseline / "
                         "--no-parity-check drop parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed as DIR/*.npy (dump_outputs: the frame and its ray counts)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def spawn_ranks(n):
    """--gpus N > 1 without a launcher: start torch.distributed.run as a CHILD process (never exec: a process that
    has initialised the GPU must not be replaced, and this one has not touched it yet) and return its exit code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL needs it on this host driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def prepare_rank_env(world):
    """What a rank needs in its environment BEFORE torch / HIP are loaded, however it was started - by spawn_ranks above or by
    the driver's own `python -m torch.distributed.run ... bench.py` (which sets nothing of this).  The pool's host driver only
    supports dmabuf IPC: without HSA_ENABLE_IPC_MODE_LEGACY=0 RCCL's bootstrap fails with `hipIpcGetMemHandle: invalid argument`
    on the first multi-rank launch.  setdefault: an operator's explicit value wins."""
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")


def rank_plumbing(args, rank, local_rank, world):
    """The rank / tile / sample plumbing of main(), as data (no torch, no GPU touched): which tiles this rank owns under the
    (tx + ty) % N deal (the same distributed.owned_tile_ids the gather assembles the frame with) and how many samples a step
    adds.  tests/test_bench_host.py starts bench.py both ways - as the driver does, under torch.distributed.run, and
    self-spawned - and compares what the ranks report."""
    import hashlib
    from jaderaytracerendering_amd import distributed as D
    width, height = (3840, 2160) if args.config == "C5" else (1920, 1080)
    width, height = args.width or width, args.height or height
    owned = [int(t) for t in D.owned_tile_ids(width, height, rank, world)]
    return {"rank": rank, "local_rank": local_rank, "world": world, "gpus": args.gpus, "spp_per_step": args.spp_per_step * world,
            "steps": args.steps, "warmup": args.warmup, "dist_backend": args.dist_backend, "width": width, "height": height,
            "owned_tiles": len(owned), "owned_tiles_sha": hashlib.sha256(repr(owned).encode()).hexdigest()[:16], "first_tiles": owned[:4],
            "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), "MASTER_ADDR": os.environ.get("MASTER_ADDR"),
            "torch_loaded": "torch" in sys.modules}


def profile_json(name):
    try:
        return json.load(open(os.path.join(ROOT, "profiles", name)))
    except Exception:
        return None


def csrc_hash(read=None):
    """sha256 over the CODE the device side is built from - csrc/*.h, *.hip and the two shared headers with comments and blank
    space stripped, so that editing a comment does not orphan the counter files (tools/summarize_prof.py stamps them with it)."""
    import glob
    import hashlib
    import re
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "jaderaytracerendering_amd", "csrc", "*.h*"))) + [os.path.join(ROOT, "include", n) for n in ("jade_fpmath.h", "jade_rt.h")]
    for f in files:
        text = (read or (lambda path: open(path, errors="replace").read()))(f)
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)      # block comments
        text = re.sub(r"//[^\n]*", " ", text)                    # line comments (no string literal of these sources holds "//")
        text = re.sub(r"\s+", " ", text).strip()
        h.update(os.path.basename(f).encode())
        h.update(text.encode())
    return h.hexdigest()[:16]


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))
    args.gpus = world
    prepare_rank_env(world)
    if os.environ.get("JADE_BENCH_PLUMBING_ONLY"):   # tests/test_bench_host.py: what a rank started by the driver's launcher sees, no GPU touched
        print(json.dumps(rank_plumbing(args, rank, local_rank, world)), flush=True)
        return

    import torch
    import torch.distributed as dist

    import jaderaytracerendering_amd as J
    from jaderaytracerendering_amd import _abi, backend as B, distributed as D, host as H

    hip = J.hip()  # raises if the HIP extension is missing: no fallback
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (torch.cuda.is_available() is False)")
    rehearsal = args.dist_backend == "gloo"
    if rehearsal:
        local_rank = 0  # every rank shares GPU 0; collectives go through host memory
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    cdev = torch.device("cpu")  # where the control plane's payloads live (a few doubles per rank)
    # Two process groups (round 4).  The control plane - the barriers that bracket the timed region and the reduction of the ranks'
    # counts into the line - runs over gloo: the path has NO data-path collective (tiles are independent), so the whole-job figure
    # must not depend on whether RCCL's bootstrap likes this host.  The path's one exchange step, the frame gather, goes over RCCL
    # (device buffers, xGMI) through a group of its own, brought up and exercised HERE, before any clock runs; if that fails on any
    # rank, every rank agrees (over gloo) to gather through host memory instead, and the line says so (`exchange`).
    exchange = {"backend": None, "rccl_error": None}
    rccl_group = None
    if world > 1:
        import datetime
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", timeout=datetime.timedelta(minutes=20))
        ok = 1.0
        if rehearsal and not os.environ.get("JADE_BENCH_TRY_RCCL"):
            ok, exchange["rccl_error"] = 0.0, "rehearsal: the ranks share one GPU"
        else:
            try:
                rccl_group = dist.new_group(backend="nccl", timeout=datetime.timedelta(minutes=5), device_id=dev)
                probe = torch.ones(1, device=dev)
                dist.all_reduce(probe, group=rccl_group)
                torch.cuda.synchronize()
                if float(probe.item()) != float(world):
                    raise RuntimeError("RCCL all_reduce of ones over %d ranks returned %r" % (world, probe.item()))
            except Exception as e:  # noqa: BLE001 (whatever RCCL's bring-up raises: the bench goes on without it)
                ok, exchange["rccl_error"] = 0.0, "%s: %s" % (type(e).__name__, str(e)[:300])
        agreed = torch.tensor([ok], dtype=torch.float64)
        dist.all_reduce(agreed, op=dist.ReduceOp.MIN)  # (gloo) one rank without RCCL = nobody uses it
        if agreed.item() < 1.0:
            rccl_group = None
            exchange["rccl_error"] = exchange["rccl_error"] or "another rank could not bring RCCL up"
        exchange["backend"] = "rccl" if rccl_group is not None else "gloo (host memory)"

    t0 = time.time()
    dev_build_ms = None
    if args.bvh != "sah":
        sb = J.SceneBuilder()
        cfg = sb.config(args.config)
        hs, dev_build_ms = sb.build_device_bvh(hip, args.bvh, leaf_size=args.bvh_leaf or (3 if args.bvh == "ploc" else 8), device_id=local_rank)
        sb.close()
    else:
        hs, cfg = J.build_config(args.config)
    build_s = time.time() - t0
    width = args.width or cfg.width
    height = args.height or cfg.height
    part_world, part_rank = world, rank
    if args.virtual_ranks > 1 and world == 1:
        part_world, part_rank = args.virtual_ranks, args.virtual_rank % args.virtual_ranks
    spp_step = args.spp_per_step * part_world  # weak scaling: fixed work per GPU per step
    walk_name = "reference" if args.reference_walk else (args.walk or "early_exit")
    walk = {"reference": _abi.WALK_REFERENCE, "early_exit": _abi.WALK_EARLY_EXIT, "cached": _abi.WALK_EARLY_EXIT_CACHED}[walk_name]
    params = B.make_params(width, height, spp_step, list(cfg.eye), list(cfg.camera), tile_rank=part_rank,
                           tile_nranks=part_world, device_id=local_rank, walk=walk)
    if rehearsal and world > 1:  # ranks share one GPU: each may hold its share of the memory, not 60 % of what is free
        params.max_state_bytes = int(0.6 * torch.cuda.mem_get_info(local_rank)[0] / world)
    if args.max_state_gb > 0:
        params.max_state_bytes = int(args.max_state_gb * 1e9)
    # the render is announced with every sample it will get (warm-up + timed steps): the backend sizes its records per
    # pixel and partial sums from it (jade_rt.h)
    params.spp = spp_step * (args.warmup + args.steps)
    scene = hip.scene(hs, device_id=local_rank)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    scene.begin(params)
    state = {"records_per_pixel": scene.query(_abi.Q_RECORDS_PER_PIXEL), "state_bytes": scene.query(_abi.Q_STATE_BYTES),
             "sum_lanes": scene.query(_abi.Q_SUM_LANES), "max_state_bytes": int(params.max_state_bytes) or None}
    st_w = _abi.Stats()
    for _ in range(args.warmup):
        scene.step(spp_step, st_w)
    scene.flush(st_w)  # the warm-up's last paths finish outside the timed region ...
    st = _abi.Stats()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        scene.step(spp_step, st)  # synchronous; a step may hand its last few paths to the next one (jade_rt.h)
    syncs_in_steps = int(st.host_syncs)
    launches_in_steps = int(st.trace_launches)
    tf = time.perf_counter()
    scene.flush(st)  # ... and the timed steps' own inside it: every sample of the K steps is done before the clock stops
    flush_ms = (time.perf_counter() - tf) * 1e3
    barrier()
    dt = time.perf_counter() - t0

    # the single exchange step: gather the framebuffer on rank 0
    n_owned = hip.owned_tile_count(width, height, part_rank, part_world)
    tiles = torch.empty((n_owned, D.TILE, D.TILE, 3), dtype=torch.float32, device=dev)
    barrier()
    g0 = time.perf_counter()
    scene.resolve_tiles_device(tiles.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if world > 1:
        frame = D.gather_framebuffer(tiles, width, height, group=rccl_group) if rccl_group is not None else D.gather_framebuffer(tiles.cpu(), width, height)
    else:
        frame = None
    barrier()
    gather_ms = (time.perf_counter() - g0) * 1e3
    if world == 1 and part_world == 1:
        frame = D.gather_framebuffer(tiles, width, height)
    frame_ok, frame_sha, frame_np = True, None, None
    if rank == 0 and frame is not None:
        frame_ok = bool(torch.isfinite(frame).all().item()) and tuple(frame.shape) == (height, width, 3)
        import hashlib
        frame_np = frame.detach().cpu().contiguous().numpy()
        frame_sha = hashlib.sha256(frame_np.tobytes()).hexdigest()[:32]  # the gathered linear frame, bit for bit

    cls_keys = ("rays_primary", "rays_shadow", "rays_env", "rays_indirect", "rays_mirror", "rays_refract")
    vals = torch.tensor([float(st.rays_primary + st.rays_secondary), float(st.nodes_visited), float(st.tris_tested),
                         st.trace_ms, float(st.trace_launches), float(st.samples)] + [float(getattr(st, k)) for k in cls_keys],
                        dtype=torch.float64, device=cdev)
    tmax = torch.tensor([dt], dtype=torch.float64, device=cdev)
    if world > 1:
        dist.all_reduce(vals, op=dist.ReduceOp.SUM)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    rays_all = float(vals[0].item())

    if rank == 0 and args.dump_outputs:
        if frame_np is None:  # --virtual-ranks: this rank's share of the frame, the other ranks' tiles left zero
            frame_np = B.assemble_tiles(tiles.cpu().numpy(), width, height, part_rank, part_world)
        dump_outputs(args.dump_outputs, frame_np, vals[[0, 5] + list(range(6, 6 + len(cls_keys)))].numpy())

    full = args.full and rank == 0 and world == 1   # the side measurements and checks of --full (one rank, after the timed steps)
    parity_frame = None
    if full and part_world == 1 and not args.no_cpu_baseline and not args.no_parity_check:
        parity_frame = scene.resolve()   # (rgb, bgr8) of the frame the timed region finished: host copies, outside the clock
    # The same steps with the other walks, outside the timed region and with the SAME step and warm-up counts (a side run
    # of two steps weighs its flush differently): the reference's walk - what the early exits are worth, and the V / T per ray of the
    # REFERENCE traversal that SURVEY 8(d)'s algorithmic bytes are defined by - and early exits without the occluder cache.
    def side_run(side_walk, what):
        rp = type(params).from_buffer_copy(params)
        rp.walk = side_walk
        k_steps = args.side_steps or args.steps
        rp.spp = spp_step * (args.warmup + k_steps)
        scene.begin(rp)
        rw = _abi.Stats()
        for _ in range(args.warmup):
            scene.step(spp_step, rw)
        scene.flush(rw)
        rs = _abi.Stats()
        torch.cuda.synchronize()
        r0 = time.perf_counter()
        for _ in range(k_steps):
            scene.step(spp_step, rs)
        scene.flush(rs)   # inside the clock, as in the timed region above
        rdt = time.perf_counter() - r0
        r_rays = float(rs.rays_primary + rs.rays_secondary)
        r_trace = max(float(r_rays - rs.rays_inline - rs.rays_tail), 1.0)
        return {"value": r_rays / rdt / 1e6, "unit": "Mray/s", "ms_per_step": rdt / k_steps * 1e3, "steps": k_steps, "warmup": args.warmup,
                "k_trace_ms_per_step": rs.trace_ms / k_steps, "k_trace_Mray_per_s": r_trace / (rs.trace_ms * 1e-3) / 1e6 if rs.trace_ms else None,
                "nodes_per_ray_k_trace": float(rs.nodes_visited - rs.nodes_inline - rs.nodes_tail) / r_trace,
                "tris_per_ray_k_trace": float(rs.tris_tested - rs.tris_inline - rs.tris_tail) / r_trace,
                "what": what}

    ref_walk = early_walk = None
    if full and not args.no_extras:
        if walk != _abi.WALK_REFERENCE:
            ref_walk = side_run(_abi.WALK_REFERENCE, "this rank's share of the frame, same steps and warm-up as the timed region, jade_render_params.walk = "
                                "JADE_WALK_REFERENCE (nodes_visited / tris_tested equal the oracle's); the flush inside its clock, outside the timed region")
        if walk == _abi.WALK_EARLY_EXIT_CACHED:
            early_walk = side_run(_abi.WALK_EARLY_EXIT, "the same with JADE_WALK_EARLY_EXIT: early exits, no occluder cache")

    if rank == 0:
        # rooflines of the dominant kernel (k_trace) on THIS rank
        # k_trace traces what the fused first-pass kernel (k_light: camera rays, floor mirrors) did not trace itself
        rays_rank = float(st.rays_primary + st.rays_secondary - st.rays_inline - st.rays_tail)   # (k_tail: the render's last paths, one launch of its own)
        v_trace, t_trace = float(st.nodes_visited - st.nodes_inline - st.nodes_tail), float(st.tris_tested - st.tris_inline - st.tris_tail)   # node records read / triangle tests made
        # bytes the REFERENCE traversal needs for k_trace's rays - with early exits the kernel reads fewer, so V and T
        # per ray come from the reference-walk steps above (the same rays: the frame is the same)
        if ref_walk is not None:
            alg_trace = (40.0 * ref_walk["nodes_per_ray_k_trace"] + 36.0 * ref_walk["tris_per_ray_k_trace"]) * rays_rank
        else:
            alg_trace = 40.0 * v_trace + 36.0 * t_trace
        alg_light = 40.0 * st.nodes_inline + 36.0 * st.tris_inline
        launches = max(int(st.trace_launches), 1)
        trace_s = st.trace_ms * 1e-3
        # per-ray counter figures exist for the configurations that were profiled (same scene, frame and BVH) - and for one build
        key = {"C3": "C3", "C4": "C3", "C5": "C5"}.get(args.config) if (args.bvh == "sah" and not args.width and not args.height) else None
        ctr_file = profile_json("k_trace_counters.json") or {}
        tree_sha = csrc_hash()
        stale = ctr_file.get("csrc_sha") != tree_sha
        ctr = None if stale else ctr_file.get(key)
        common = {"kernel": "k_trace", "avg_launch_ms": st.trace_ms / launches, "launches": launches}

        def roof_of(bound, per_ray, scale, peak, unit, extra=None):
            r = {"bound": bound, "achieved": None, "peak": peak, "unit": unit, "frac": None, "traffic": None}
            r.update(common)
            if per_ray and trace_s > 0:
                r["achieved"] = per_ray * rays_rank / trace_s / scale
                r["frac"] = r["achieved"] / peak
            if extra:
                r.update(extra)
            return r

        c = ctr or {}
        hbm_per_ray = c.get("hbm_bytes_per_ray")
        rooflines = {
            "valu": roof_of("valu", c.get("valu_lane_ops_per_ray"), 1e12, VALU_PEAK_TLANEOPS, "Tlane-op/s",
                            {"valu_wave_insts_per_ray": c.get("valu_wave_insts_per_ray"), "lanes_per_valu_inst_of_64": c.get("lanes_per_valu_inst"),
                             "issue_busy_of_2": c.get("valu_busy"), "valu2_share_of_valu_time": c.get("valu2_share_of_valu_time"),
                             "frac_of_one_instruction_per_4_clocks": None,
                             "note": "peak = one wave64 VALU instruction per SIMD per 2 clocks (MI355X_MICROARCH.md: 2 cycles on a SIMD-32, which "
                                     "takes two or more waves per SIMD; ONE wave's own stream issues one per 4); issue_busy_of_2 = 4 x SQ_ACTIVE_INST_VALU / SIMD-cycles"}),
            "valu_issue": roof_of("valu_issue", c.get("valu_wave_insts_per_ray"), 1e9, VALU_ISSUE_PEAK_GINST, "Ginst/s",
                                  {"valu_wave_insts_per_ray": c.get("valu_wave_insts_per_ray"), "valu_busy_profiled": c.get("valu_busy"),
                                   "note": "wave64 VALU instructions issued per second against one per SIMD per 4 clocks: the calibrated issue rate of every "
                                           "instruction kind but unpacked fp32 add / mul / fma and v_mov (profiles/valu_calibration.json); idle lanes are "
                                           "not counted against the kernel here (they are in the 'valu' roof's lane-operations).  valu_busy_profiled = 4 x "
                                           "instructions per SIMD per clock over the profiled run's own clocks"}),
            "l2": roof_of("l2", (c.get("l2_requests_per_ray") or 0) * 64.0, 1e9, L2_GATHER_PEAK_GBS, "GB/s",
                          {"l2_requests_per_ray": c.get("l2_requests_per_ray"), "l2_hit_rate": c.get("l2_hit_rate"),
                           "note": "(TCC_HIT_sum + TCC_MISS_sum) x 64 B per ray; peak = what the guide measures for gathers served by the XCDs' L2s (16.8-18.8 TB/s)"}),
            "hbm": roof_of("hbm", hbm_per_ray, 1e9, HBM_PEAK_GBS, "GB/s",
                           {"fetch_size_factor": c.get("fetch_size_factor"), "note": "FETCH_SIZE x fetch_size_factor + WRITE_SIZE per ray; the factor is what "
                            "tools/fetch_calib measured for 64-B gathers (profiles/fetch_calibration.json); Infinity-Cache hits are inside FETCH_SIZE"}),
        }
        if rooflines["valu"]["frac"] is not None:  # the other reading of the VALU roof: one instruction per SIMD per 4 clocks
            rooflines["valu"]["frac_of_one_instruction_per_4_clocks"] = 2.0 * rooflines["valu"]["frac"]
        for r in rooflines.values():
            r["counters_from"] = c.get("source")
            if r["bound"] == "hbm" and hbm_per_ray:
                r["traffic"] = hbm_per_ray * rays_rank / launches
        ranked = [r for r in rooflines.values() if r["frac"] is not None]
        roof = dict(max(ranked, key=lambda r: r["frac"])) if ranked else dict(rooflines["hbm"])
        if hbm_per_ray:
            roof["traffic"] = hbm_per_ray * rays_rank / launches   # measured HBM-side bytes per launch, whatever the bound
        roof.update({
            "trace_share_of_step_time": trace_s / (st.kernel_ms * 1e-3) if st.kernel_ms else None,
            # what a profiler sees for the same command: every k_trace launch of the process, warm-up included (launches count
            # the empty ones behind the end of a step's batch too - they are launches, of a few microseconds)
            "launches_incl_warmup": launches + int(st_w.trace_launches),
            "avg_launch_ms_incl_warmup": (st.trace_ms + st_w.trace_ms) / max(launches + int(st_w.trace_launches), 1),
            "rays_per_launch": rays_rank / launches, "rays_traced_by_this_kernel": rays_rank,
            "Mray_per_s_of_this_kernel": rays_rank / trace_s / 1e6 if trace_s > 0 else None,
            "algorithmic_bytes_per_launch": alg_trace / launches,
            "algorithmic_GBps": alg_trace / trace_s / 1e9 if trace_s > 0 else None,
            # whose V and T priced the algorithmic bytes: the reference walk's side run (--full), else this run's own walk
            "algorithmic_walk": "reference" if ref_walk is not None else walk_name,
            "counters_build": ctr_file.get("csrc_sha"), "tree_build": tree_sha,
            "counters_stale": ("profiles/k_trace_counters.json was cut from another build of csrc/ (%s, tree %s): fractions withheld"
                               % (ctr_file.get("csrc_sha"), tree_sha)) if stale else None})
        out = {
            "metric": "Mray/s (primary+secondary)",
            "value": rays_all / dt / 1e6,
            "unit": "Mray/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{args.config}: jade statue stand-in ({hs.n_triangles:,} triangles, {args.bvh.upper()} BVH), {width}x{height}, "
                            f"{spp_step} spp per step, tiles dealt over {world} GPU(s)",
                "spp_per_step": spp_step, "width": width, "height": height, "triangles": hs.n_triangles,
                "bvh_nodes": hs.n_nodes, "bvh_depth": hs.bvh_depth, "parallelism": f"tiles{world}",
                "walk": walk_name,
            },
            # the same steps with every query walked to the end as the reference does (null without --full, or with --reference-walk / --no-extras)
            "reference_walk": ref_walk,
            "value_reference_walk": ref_walk["value"] if ref_walk else (None if walk != _abi.WALK_REFERENCE else rays_all / dt / 1e6),
            # ... and with early exits but no occluder cache (null unless the timed region ran with the cache)
            "early_exit_walk": early_walk,
            "value_early_exit_walk": early_walk["value"] if early_walk else (rays_all / dt / 1e6 if walk == _abi.WALK_EARLY_EXIT else None),
            # JADE_WALK_EARLY_EXIT_CACHED: yes/no queries (shadow + environment rays) the cached subtrees answered without a walk from the root
            "occluder_cache": {"answered": float(st.rays_cached), "share_of_shadow_and_env_rays": float(st.rays_cached) / max(float(st.rays_shadow + st.rays_env), 1.0)}
            if walk == _abi.WALK_EARLY_EXIT_CACHED else None,
            "virtual_ranks": part_world if part_world != world else None,
            "rehearsal_all_ranks_on_one_gpu": True if rehearsal else None,
            "rays": rays_all,
            "samples": float(vals[5].item()),
            "rays_incl_warmup_this_rank": float(st.rays_primary + st.rays_secondary + st_w.rays_primary + st_w.rays_secondary),
            "rays_k_trace_incl_warmup_this_rank": float(st.rays_primary + st.rays_secondary - st.rays_inline - st.rays_tail + st_w.rays_primary
                                                        + st_w.rays_secondary - st_w.rays_inline - st_w.rays_tail),
            # the step by kernel on this rank: k_light (fused first pass: light samples traced and shaded in one kernel),
            # k_trace (everything else that is traced), the rest = k_shade / k_arm / gaps
            "kernels": {"k_light": {"ms_per_step": st.light_ms / max(args.steps, 1), "rays": float(st.rays_inline),
                                    "Mray_per_s": st.rays_inline / (st.light_ms * 1e-3) / 1e6 if st.light_ms else None,
                                    "nodes_per_ray": st.nodes_inline / max(float(st.rays_inline), 1.0), "tris_per_ray": st.tris_inline / max(float(st.rays_inline), 1.0),
                                    "algorithmic_bytes_per_ray": alg_light / max(float(st.rays_inline), 1.0),
                                    "algorithmic_GBps": alg_light / (st.light_ms * 1e-3) / 1e9 if st.light_ms else None},
                        "k_trace": {"ms_per_step": st.trace_ms / max(args.steps, 1), "rays": rays_rank,
                                    "Mray_per_s": rays_rank / trace_s / 1e6 if trace_s > 0 else None,
                                    "nodes_per_ray": v_trace / max(rays_rank, 1.0), "tris_per_ray": t_trace / max(rays_rank, 1.0),   # read / made by this walk
                                    "algorithmic_bytes_per_ray": alg_trace / max(rays_rank, 1.0),                                   # of the reference's walk
                                    "algorithmic_GBps": alg_trace / trace_s / 1e9 if trace_s > 0 else None},
                        # k_tail: ONE launch that shades and traces the last paths of the render (the flush; small renders: of every step)
                        "k_tail": {"ms": st.tail_ms, "launches": int(st.tail_launches), "rays": float(st.rays_tail)},
                        "device_ms_per_step": st.kernel_ms / max(args.steps, 1),
                        "rest_ms_per_step": (st.kernel_ms - st.trace_ms - st.light_ms - st.tail_ms) / max(args.steps, 1)},
            "state": state,
            "rays_by_call_site": {k[5:]: float(vals[6 + i].item()) for i, k in enumerate(cls_keys)},
            "gather_ms": gather_ms,
            # N > 1: what carried the frame gather - "rccl" (device buffers), or "gloo (host memory)" with the reason RCCL was not used;
            # barriers and the reduction of the ranks' counts always run over gloo (no collective is inside the timed region)
            "exchange": exchange if world > 1 else None,
            "frame_ok": frame_ok,
            "frame_sha256": frame_sha,   # equal for any number of ranks at equal total samples (tests/test_gpu_bench.py)
            # host waits for the device: per step (the fused first pass, then ONE batch of up to 32 shade / trace passes that
            # stops itself at the carry-over point), and in the flush that finishes the last paths of the render
            "host_syncs_per_step": syncs_in_steps / max(args.steps, 1),
            "host_syncs_in_final_flush": int(st.host_syncs) - syncs_in_steps,
            # the flush that finishes the longest paths of the K steps (inside the timed region, once per render)
            "final_flush": {"ms": flush_ms, "k_trace_launches": int(st.trace_launches) - launches_in_steps},
            "scene_build_s": build_s,
            "bvh": args.bvh, "device_bvh_ms": dev_build_ms,
            "nodes_per_ray": float(vals[1].item()) / rays_all, "tris_per_ray": float(vals[2].item()) / rays_all,
            "roofline": roof,
            "rooflines": rooflines,
            # the resource with the largest share of its roof (null when the counter file belongs to another build)
            "binding": roof["bound"] if roof.get("frac") is not None else None,
        }
        if full and part_world == 1 and not args.no_extras and args.config in ("C2", "C3", "C4"):
            out["statue_closeup"] = closeup(scene, hip, B, H, _abi, cfg, width, height, args.spp_per_step, walk)
        if full and part_world == 1 and not args.no_extras and args.config in ("C3", "C4"):
            out["glass_statue"] = glass_statue(hip, J, B, _abi, width, height, args.spp_per_step, walk, check=not args.no_cpu_baseline)
        if full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(hs, cfg, width, height, args.cpu_spp)
            if parity_frame is not None:
                out["parity_check"] = parity_check(hs, cfg, width, height, int(params.spp), parity_frame, args.parity_rays)
        print(json.dumps(out), flush=True)
    scene.close()
    if world > 1:
        dist.destroy_process_group()


DUMP_BYTES = 60 << 20   # --dump-outputs writes at most this much (under 64 MB with the .npy headers)
DUMP_COUNTERS = ("rays", "samples", "rays_primary", "rays_shadow", "rays_env", "rays_indirect", "rays_mirror", "rays_refract")


def dump_outputs(out_dir, frame, counters):
    """--dump-outputs: what the timed steps computed, for comparing two builds output for output (the inputs are the same on
    every run with the same arguments: the scene is built by the host pipeline, every sample's random stream is seeded by its
    pixel and index, jade_rt.h).
      radiance.npy  float32 [H, W, 3]: the linear frame after warm-up + timed steps, as gathered on rank 0.  A frame larger than
                    the budget is written as a fixed, seeded sample of its pixels instead: radiance_sample.npy float32 [k, 3] holds
                    pixels radiance_sample_index.npy (float64, row-major y * W + x) of the frame.
      counters.npy  float64 [8]: DUMP_COUNTERS of the timed steps, summed over the ranks."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    frame = np.ascontiguousarray(frame, np.float32)
    counters = np.asarray(counters, np.float64)
    assert counters.shape == (len(DUMP_COUNTERS),)
    if frame.nbytes + counters.nbytes <= DUMP_BYTES:
        np.save(os.path.join(out_dir, "radiance.npy"), frame)
    else:
        pixels = frame.reshape(-1, 3)
        k = (DUMP_BYTES - counters.nbytes) // (pixels.itemsize * 3 + 8)
        idx = np.sort(np.random.default_rng(0).choice(len(pixels), size=k, replace=False))
        np.save(os.path.join(out_dir, "radiance_sample.npy"), pixels[idx])
        np.save(os.path.join(out_dir, "radiance_sample_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, "counters.npy"), counters)


def closeup(scene, hip, B, H, _abi, cfg, width, height, spp, walk):
    """The same scene with the camera moved in until the statue fills the frame: every pixel starts a jade path
    (BSSRDF / SSS / mirror branches, ~4 shadow + environment + indirect rays per bounce).  The headline frame is
    ~5 % statue; this is the rate on the rays it has few of.  One warm-up step, two timed steps (the faster one counts), all flushed."""
    import numpy as np
    hs = scene.host_scene
    centre = hs.vertices()[hs.tri_i32()[:, 0] == 0].reshape(-1, 3).mean(0)  # object 0 is the statue (scene_io.cpp add_jade_scene)
    forward = -np.array(cfg.camera[8:11], np.float32)                       # the view axis: M . (0, 0, -1, 0)
    eye = centre - 0.22 * forward                                           # C3 looks at it from 0.56 away
    spp = max(1, min(spp, 256))
    p = B.make_params(width, height, spp, [float(x) for x in eye], list(cfg.camera), walk=walk)
    p.spp = 3 * spp  # (announced = rendered: one warm-up step and two timed ones)
    scene.begin(p)
    w = _abi.Stats()
    scene.step(spp, w)
    scene.flush(w)
    # two timed steps, the faster one reported (and both times): a side measurement of one second each must not hang on one hiccup of
    # the box (seen once in round 4: 4.3 s of wall time for 1.03 s of kernels, every other run of the same command 2.70-2.72 Gray/s)
    runs = []
    for _ in range(2):
        st_i = _abi.Stats()
        t0 = time.perf_counter()
        scene.step(spp, st_i)
        scene.flush(st_i)
        runs.append((time.perf_counter() - t0, st_i))
    dt, st = min(runs, key=lambda r: r[0])
    rays = float(st.rays_primary + st.rays_secondary)
    return {"value": rays / dt / 1e6, "unit": "Mray/s", "spp": spp, "timed_steps_s": [r[0] for r in runs], "rays_per_sample": rays / max(st.samples, 1),
            "nodes_per_ray": st.nodes_visited / rays, "tris_per_ray": st.tris_tested / rays,
            "k_trace_Mray_per_s": rays / (st.trace_ms * 1e-3) / 1e6 if st.trace_ms else None,
            "trace_share_of_step_time": st.trace_ms / st.kernel_ms if st.kernel_ms else None,
            "camera": "C3's view direction, eye moved to 0.22 from the statue's centre (C3: 0.56)"}


def glass_statue(hip, J, B, _abi, width, height, spp, walk, check=True):
    """Config C3G: C3's frame with the statue made of DIR_REFRACT glass (refract_mode 2, PathTrace.cu:1180-1262) - the third
    material mode, whose serial chain of up to 32 internal reflections / refractions per sample no BASELINE config exercises
    (rays_by_call_site.refract is 0 in every other frame of this line).  One warm-up step, one timed step, both flushed; then the
    frame of those two steps against the oracle on three tiles (statue, floor, sky) - the checker leg, outside the clock."""
    import numpy as np
    from jaderaytracerendering_amd import host as H
    hs, cfg = J.build_config("C3G")
    spp = max(1, min(spp, 128))
    p = B.make_params(width, height, 2 * spp, list(cfg.eye), list(cfg.camera), walk=walk)
    with hip.scene(hs) as sc:
        sc.begin(p)
        w = _abi.Stats()
        sc.step(spp, w)
        sc.flush(w)
        st = _abi.Stats()
        t0 = time.perf_counter()
        sc.step(spp, st)
        sc.flush(st)
        dt = time.perf_counter() - t0
        frame = sc.resolve() if check else None
    rays = float(st.rays_primary + st.rays_secondary)
    out = {"value": rays / dt / 1e6, "unit": "Mray/s", "config": "C3G", "spp": spp, "rays_per_sample": rays / max(st.samples, 1),
           "rays_by_call_site": {k[5:]: float(getattr(st, k)) for k in ("rays_primary", "rays_shadow", "rays_env", "rays_indirect", "rays_mirror", "rays_refract")},
           "nodes_per_ray": st.nodes_visited / rays, "tris_per_ray": st.tris_tested / rays,
           "k_trace_Mray_per_s": (rays - st.rays_inline) / (st.trace_ms * 1e-3) / 1e6 if st.trace_ms else None,
           "trace_share_of_step_time": st.trace_ms / st.kernel_ms if st.kernel_ms else None, "k_trace_launches": int(st.trace_launches),
           "what": "C3's geometry, camera and frame size; statue material: reflex MIRROR, refract DIR_REFRACT, index 1.5, rate (0.9, 0.95, 0.9)"}
    if frame is not None:
        out["parity_check"] = parity_check(hs, cfg, width, height, 2 * spp, frame, 4.0e7)
    return out


def parity_check(hs, cfg, width, height, spp_total, frame, ray_budget):
    """The rendered frame against the oracle on a few tiles at the full sample count (the checker leg: the oracle is
    test infrastructure and is only ever compared WITH).  Tiles: the statue tile with the most vertices, a tile of the
    mirror floor, a sky tile, then more statue / edge tiles while the oracle's estimated rays fit the budget."""
    import ctypes
    import numpy as np
    from jaderaytracerendering_amd import backend as B, host as H
    lib = os.path.join(ROOT, "oracle", "libjade_oracle.so")
    if not os.path.exists(lib):
        return None
    rgb, bgr = frame
    tiles_x, tiles_y = (width + 15) // 16, (height + 15) // 16
    statue = H.object_tiles(hs, cfg.eye, cfg.camera, width, height, obj=0)
    by_count = sorted(statue, key=statue.get, reverse=True)
    cand = []   # (tile id, estimated rays per sample)
    if by_count:
        cand.append((by_count[0], 25.0))
        sty, stx = divmod(by_count[0], tiles_x)
        cand.append((max(sty - 14, 0) * tiles_x + stx, 2.5))                                  # the mirror floor in front of the statue
    cand.append(((tiles_y - 3) * tiles_x + 5, 1.0))                                          # sky
    if len(by_count) > 8:
        cand.append((by_count[len(by_count) // 2], 15.0))                                     # a tile the statue half covers
        cand.append((by_count[1], 25.0))
    cand.append(((tiles_y - 1) * tiles_x + tiles_x - 1, 1.0))                                # the top right corner (a partial tile at 1080p)
    chosen, cost = [], 0.0
    for tid, rps in cand:
        c = 256.0 * spp_total * rps
        if tid in chosen or (len(chosen) >= 3 and cost + c > ray_budget):
            continue
        chosen.append(tid)
        cost += c
    oracle = B.Backend(lib)
    fn = oracle.lib.jade_oracle_set_tile_filter   # checker-only export of oracle/jade_oracle.c
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    ids = np.ascontiguousarray(chosen, np.int32)
    p = B.make_params(width, height, spp_total, list(cfg.eye), list(cfg.camera), threads=usable_cores())
    t0 = time.perf_counter()
    with oracle.scene(hs) as so:
        oracle.check(fn(so._h, ids.ctypes.data, len(ids)))
        o_rgb, o_bgr, st = so.render(p)
    dt = time.perf_counter() - t0
    m = np.zeros((height, width), bool)
    for t in chosen:
        ty, tx = divmod(int(t), tiles_x)
        m[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = True
    a, b = rgb[m].astype(np.float64), o_rgb[m].astype(np.float64)
    rel = float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))
    bgr_max = int(np.abs(bgr[m].astype(np.int16) - o_bgr[m].astype(np.int16)).max())
    return {"tiles": [[int(t % tiles_x), int(t // tiles_x)] for t in chosen], "pixels": int(m.sum()), "spp": spp_total,
            "rel_l2": rel, "bgr_max": bgr_max, "ok": bool(rel <= 1e-4 and bgr_max <= 1), "tolerance": {"rel_l2": 1e-4, "bgr": 1},
            "oracle_rays": int(st.rays), "oracle_s": dt,
            "what": "the frame of this run (warm-up + timed steps, the benchmarked schedule) vs the CPU oracle on these 16x16 tiles at the same sample count"}


def usable_cores():
    """Cores this process may really use: affinity mask, capped by the cgroup CPU quota."""
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    cores = min(cores, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    cores = min(cores, max(1, q // per))
            break
        except Exception:
            continue
    return cores


def cpu_baseline(hs, cfg, width, height, spp):
    """The oracle (a port: the reference has no CPU integrator) on all host cores."""
    from jaderaytracerendering_amd import backend as B
    lib = os.path.join(ROOT, "oracle", "libjade_oracle.so")
    if not os.path.exists(lib):
        return None
    cores = usable_cores()
    oracle = B.Backend(lib)
    p = B.make_params(width, height, spp, list(cfg.eye), list(cfg.camera), threads=cores)
    with oracle.scene(hs) as so:
        t0 = time.perf_counter()
        _, _, st = so.render(p, want_rgb=False, want_bgr8=False)
        dt = time.perf_counter() - t0
    return {"value": st.rays / dt / 1e6, "unit": "Mray/s", "cores": cores, "kind": "port",
            "sample": f"same scene and camera, full {width}x{height} frame, {spp} spp ({st.rays} rays, {dt:.1f} s)"}


if __name__ == "__main__":
    main()
