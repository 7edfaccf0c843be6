#!/usr/bin/env python3
"""ELLC hot-path benchmark: Gauss-Newton iterations / second on 640x480 semi-dense alignments.

    python bench.py --gpus N --steps K --warmup W

N > 1: one rank per GPU. Either the driver starts the ranks (`python -m torch.distributed.run --nproc-per-node N ... bench.py
--gpus N ...`: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT come from the environment), or — when WORLD_SIZE is
not set — this program starts them itself: N child processes with that environment, BEFORE anything touches the GPU, rank 0's
JSON line passed through. Nothing here imports torch: the ranks meet over the library's own host-side communicator (TCP on
MASTER_ADDR:MASTER_PORT+17 — barrier, unique id, maximum of the timings) and the data path's one collective, the gather of the
resulting se(3) poses, is ncclAllGather (RCCL over xGMI) issued by the library's C entry points (ellc_gather_start / _finish).

One *step* = one pass of the hot path over one batch: the loop-closure batch in the reference's own shape
(GlobalOptimize.cpp:566) — `--batch` different keyframes, each with its own semi-dense depth map, aligned against ONE
current frame — through ellc_align_enqueue / ellc_align_fetch: mask/compaction per level, then the full {4,7,9,12}
Gauss-Newton schedule with early exit disabled so the work is deterministic (32 GN iterations per alignment), followed —
when N>1 — by the single gather of the resulting se(3) poses over RCCL. Inputs are resident in HBM before the timed region.

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement" for every field). A plain run does only what the headline needs:
set-up, warm-up, the K timed steps and the contract's fields. With --full the line also carries the roofline of the dominant
kernel, the same workload in the per-pixel bit-exact arithmetic mode (`exact_arith`, repeated in `config`), a sustained block of
>= 2000 steps, BASELINE configs[4] at 16 alignments per GPU (`c4_dense`), the depth-map kernels against their algorithmic bytes
(`depth`), the single alignment and tracked frame of configs[1] (with and without the loop-closure batch running beside it),
and the CPU port timed on this box's host cores (`cpu_baseline`, with the pose error of the GPU result against it).

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step returned to its caller (ellc_align_fetch) as
DIR/pose.npy (B x 6 f32 se(3)), DIR/iters.npy (B x levels, iterations per level, f64) and DIR/weighted.npy (B f32), and with a
gather DIR/gathered.npy (the last all-gathered result table, f32). The inputs are seeded: the same arguments give the same inputs.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_GBPS = 8000.0   # MI355X HBM3E (MI355X_MICROARCH.md)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=32, help="alignments per GPU per step")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--dense", action="store_true", help="all-pixel residuals instead of semi-dense (own frame per alignment)")
    ap.add_argument("--mode", choices=["fca", "ica"], default="fca")
    ap.add_argument("--arith", choices=["fast", "exact"], default="fast", help="arithmetic of the Gauss-Newton pixel pass and solve (cfg.arith): "
                    "fast = tolerance mode (pose <= 1e-5 vs the oracle), exact = per-pixel bit-exact mode")
    ap.add_argument("--inflight", type=int, default=16, help="batches in flight per GPU (1 .. 4 x --coalesce; 1 .. 3 with --coalesce 1), each on its own slot group")
    ap.add_argument("--coalesce", type=int, default=4, help="cfg.coalesce: full batches enqueued one after the other run side by side in one "
                    "launch sequence, up to this many (1: every batch is launched by itself, at most three in flight)")
    ap.add_argument("--early-exit", action="store_true", help="informational: the reference's early exit on (data-dependent iteration counts; "
                    "value then counts the iterations actually executed)")
    ap.add_argument("--full", action="store_true", help="after the timed region: the roofline of the dominant kernel, the sub-records and the CPU "
                    "baseline (off: a plain run prints the contract's fields only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's results as DIR/<name>.npy (rank 0)")
    ap.add_argument("--blocks", type=int, default=25, help="--full: after the timed region, this many further blocks of --steps steps, for the spread (N=1)")
    ap.add_argument("--sustained", type=int, default=2000, help="--full: after the timed region, one block of this many steps (N=1; 0: none)")
    ap.add_argument("--no-extras", action="store_true", help="--full: the roofline only (no exact_arith / c4_dense / depth / tracking sub-records)")
    ap.add_argument("--trace-only", action="store_true", help="stop after the timed region (kernel traces of exactly the timed workload)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: no CPU baseline")
    ap.add_argument("--gather-at-1", action="store_true", help="N=1 only: run the per-batch gather all the same (RCCL communicator of one rank through "
                    "the library's C entry points): what the exchange costs the loop, measured on one GPU")
    ap.add_argument("--backend", choices=["nccl", "gloo", "tcp"], default="nccl", help="N>1: transport of the gather of the poses. nccl = RCCL "
                    "(ncclAllGather over xGMI, one GPU per rank); gloo / tcp = the same entry points over the library's TCP transport "
                    "(host memory): only to rehearse several ranks on ONE GPU, where RCCL refuses two ranks on a device")
    ap.add_argument("--cpu-seconds", type=float, default=4.0, help="wall-time budget of each CPU baseline variant")
    ap.add_argument("--rehearse-launcher", action="store_true", help="no GPU work: start the ranks, run the control plane (barrier, id broadcast, "
                    "max) and a few pipelined gathers of stand-in result tables over the TCP transport, print what each rank saw (CPU test of the launcher)")
    ap.add_argument("--device-warmup", type=int, default=200, help="untimed steps run once before the --warmup steps (part of the setup, like the "
                    "graph-capture rehearsal; 0: none)")
    ap.add_argument("--streams", type=int, default=3, help="diagnostic: batch streams the loaded library build has (ELLC_STREAMS)")
    ap.add_argument("--no-affinity", action="store_true", help="N>1: do not pin the rank to its share of the host's CPUs")
    ap.add_argument("--cache-records", action="store_true", help="diagnostic only (NOT the contract's workload): cfg.cache_records on the main workload — the compact "
                    "lists are kept with the keyframe slots, so the timed steps contain no compaction at all: the ceiling of what hiding it can give")
    ap.add_argument("--lib", default=None, help="diagnostic A/B only: load this build of the library instead of csrc/libellc_hip.so")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


def spawn_ranks(a):
    """--gpus N > 1 without a launcher: start N ranks of this very command (before this process has loaded the library or
    touched a GPU), pass rank 0's output through, fail if any rank fails. The children find WORLD_SIZE set and run main()."""
    import socket
    port = 0
    for _ in range(64):   # MASTER_PORT such that the two ports the ranks really bind (control plane + 17, TCP gather + 18) are free now
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
            sk.bind(("127.0.0.1", 0))
            cand = sk.getsockname()[1]
        ok = cand + 18 < 65536
        for off in (17, 18):
            if not ok:
                break
            with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
                try:
                    sk.bind(("127.0.0.1", cand + off))
                except OSError:
                    ok = False
        if ok:
            port = cand
            break
    if not port:
        sys.stderr.write("bench.py: no free rendezvous ports found\n")
        return 1
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    pending = list(procs)
    while pending:
        for p in list(pending):
            code = p.poll()
            if code is None:
                continue
            pending.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in pending:   # a rank failed: the others would wait for it until their time-outs
                    q.terminate()
        time.sleep(0.05)
    return rc


class Control:
    """The ranks' control plane (never the data path): barrier, rank 0's 128-byte RCCL id to everyone, maximum of a number — each
    one gather of host memory over the library's TCP communicator (ellc_comm_init_tcp). world == 1: nothing to do."""

    def __init__(self, sharding, world, rank, host_only=False):
        self.world, self.rank = world, rank
        self.comm = None
        if world > 1:
            port = int(os.environ.get("MASTER_PORT", "29500")) + 17
            self.comm = sharding.Comm(world, rank, max_total=8 * world, transport="tcp", host=os.environ.get("MASTER_ADDR", "127.0.0.1"), port=port,
                                      host_only=host_only)

    def _gather(self, rows_per_rank, mine):
        import numpy as np
        return self.comm.gather(rows_per_rank * self.world, np.asarray(mine, np.float32).reshape(rows_per_rank, 8))

    def barrier(self):
        if self.comm is not None:
            self._gather(1, [0.0] * 8)

    def all(self, x):
        """every rank's x (an f64 as two f32 words, moved bit for bit), in rank order"""
        if self.comm is None:
            return [float(x)]
        import numpy as np
        rec = np.zeros(8, np.float32)
        rec[:2] = np.array([x], np.float64).view(np.float32)
        t = self._gather(1, rec)
        return [float(np.ascontiguousarray(t[r, :2]).view(np.float64)[0]) for r in range(self.world)]

    def max(self, x):
        return max(self.all(x))

    def all_text(self, text):
        """every rank's short string (<= 63 bytes: two records of the gather, moved bit for bit), in rank order"""
        if self.comm is None:
            return [text]
        import numpy as np
        raw = text.encode()[:63].ljust(64, b"\0")
        t = self._gather(2, np.frombuffer(raw, np.uint8).view(np.float32))
        return [np.ascontiguousarray(t[2 * r:2 * r + 2]).tobytes().split(b"\0")[0].decode(errors="replace") for r in range(self.world)]

    def broadcast_id(self, make):
        """rank 0's ellc_comm_unique_id bytes on every rank (128 bytes = 4 records of the gather, moved bit for bit)."""
        import numpy as np
        if self.comm is None:
            return make()
        mine = np.frombuffer(make() if self.rank == 0 else bytes(128), np.uint8).view(np.float32)
        return self._gather(4, mine)[:4].tobytes()

    def close(self):
        if self.comm is not None:
            self.comm.close()


class Workload:
    """G slot groups of B keyframes + one frame each, resident on the device; step s works on group s % G."""

    def __init__(self, api, a, scenes, arith, dev_index, W=None, H=None, L=None, B=None, sched=None, early_exit=None, G=None, shared_frame=True,
                 coalesce=None, prime=None, share_kf=False, cache_records=0, diag=False, upload_groups=None):
        """diag: the context lives in libellc_hip_diag.so (the measurement hooks of include/ellc_abi_diag.h; same kernels, same launch
        paths, same configuration, hence the same grids) with only the first upload_groups slot groups filled and nothing rehearsed:
        what level0_kernel() times the dominant kernel on."""
        self.api = api
        self._init_args = dict(a=a, scenes=scenes, arith=arith, dev_index=dev_index, W=W, H=H, L=L, B=B, sched=sched, early_exit=early_exit, G=G,
                               shared_frame=shared_frame, coalesce=coalesce, share_kf=share_kf, cache_records=cache_records)
        self.W, self.H, self.L = W or a.width, H or a.height, L or a.levels
        self.B = B or a.batch
        self.coalesce = max(1, min(4, a.coalesce if coalesce is None else coalesce))
        self.G = G or max(1, min((a.streams + 1) * self.coalesce if self.coalesce > 1 else a.streams, a.inflight))
        self.sched = sched or [4, 7, 9, 12, 12, 12, 12, 12][:self.L]
        fx, fy, cx, cy = scenes[0]["intrinsics"]
        B, G = self.B, self.G
        self.shared = shared_frame
        self.cfg = api.default_config(self.W, self.H, self.L, fx=fx, fy=fy, cx=cx, cy=cy, early_exit=int(a.early_exit if early_exit is None else early_exit),
                                      max_iter=self.sched, max_keyframes=G * B, max_frames=(G if shared_frame else G * B), max_batch=B, device=dev_index,
                                      concurrent_batches=G, coalesce=self.coalesce, cache_records=int(cache_records),
                                      arith=api.ARITH_FAST if arith == "fast" else api.ARITH_EXACT)
        self.ctx = api.Context(self.cfg, diag=diag)
        self.mode = api.MODE_FCA if a.mode == "fca" else api.MODE_ICA
        for g in range(G if upload_groups is None else min(G, upload_groups)):
            if shared_frame:
                self.ctx.frame_upload(g, scenes[0]["cur_image"])
            for b in range(B):
                p = scenes[b % len(scenes)]
                self.ctx.keyframe_upload(g * B + b, p["kf_image"])
                self.ctx.keyframe_set_depth(g * B + b, p["depth0"], p["var0"])
                if not shared_frame:
                    self.ctx.frame_upload(g * B + b, p["cur_image"])
                if a.mode == "ica":
                    for l in range(self.L):
                        self.ctx.keyframe_set_weights(g * B + b, l, np.full((self.H >> l, self.W >> l), 0.03, np.float32), 1)
        self.kf = [np.arange(B, dtype=np.int32) + (0 if share_kf else g * B) for g in range(G)]   # share_kf: every batch aligns the SAME keyframes
        self.fr = [np.full(B, g, np.int32) if shared_frame else self.kf[g] for g in range(G)]
        # set-up, not warm-up: launch sequences are captured into hipGraphs on first use, one per (buffer set, batches in the group);
        # a rehearsal of the step counts that will be run captures every one the measured runs replay (like the uploads above)
        if not diag:
            for n in sorted(set([G] + [int(x) for x in (prime or []) if x > 0])):
                self.run(n)

    def run(self, nsteps, on_fetch=None):
        """nsteps steps, software-pipelined through the asynchronous API: up to G batches in flight, each on its own stream and
        slot group; every batch is fetched (and, N>1, gathered) before this returns."""
        ctx, G, B = self.ctx, self.G, self.B
        pose = iters = wgt = None
        for s in range(min(G, nsteps)):
            ctx.align_enqueue(self.kf[s % G], self.fr[s % G], mode=self.mode)
        for s in range(nsteps):
            pose, iters, wgt = ctx.align_fetch(B)
            if s + G < nsteps:
                ctx.align_enqueue(self.kf[(s + G) % G], self.fr[(s + G) % G], mode=self.mode)
            if on_fetch is not None:
                on_fetch(pose, iters, wgt)
        return pose, iters, wgt

    def timed(self, nsteps):
        self.ctx.sync()
        t0 = time.perf_counter()
        pose, iters, _ = self.run(nsteps)
        self.ctx.sync()
        return time.perf_counter() - t0, pose, iters

    def diag_twin(self):
        """This workload's twin in libellc_hip_diag.so (the shipping library exports no measurement hooks): same configuration — so
        the same grids and launches — and the same scenes in the slot groups of one launch group."""
        if self.ctx.diag:
            return self
        if getattr(self, "_twin", None) is None:
            self._twin = Workload(self.api, diag=True, upload_groups=min(self.coalesce, self.G), **self._init_args)
        return self._twin

    def level0_kernel(self, reps=50):
        """The level-0 launch as the timed region issues it: over the alignments of one launch group (coalesce batches side by side).
        HIP events on the library's stream around a replayed graph of `reps` launches (ellc_profile_gn_kernel, include/ellc_abi_diag.h)."""
        tw = self.diag_twin()
        k = min(self.coalesce, self.G)
        # (the twin's set-up — uploads — lets the device idle: the same launches, untimed, bring it back to its working state first, as
        # tools/profile_kernel.py's --device-warmup does and as the timed region's own warm-up steps do for `value`)
        tw.ctx.profile_gn_kernel(np.concatenate(self.kf[:k]), np.concatenate(self.fr[:k]), 0, reps=300)
        ms, alg, V = tw.ctx.profile_gn_kernel(np.concatenate(self.kf[:k]), np.concatenate(self.fr[:k]), 0, reps=reps)
        gbps = alg / (ms * 1e-3) / 1e9
        return {"avg_launch_ms": ms, "alignments_per_launch": int(k * self.B), "algorithmic_bytes_per_launch": alg, "valid_pixels_per_launch": V,
                "achieved": gbps, "frac": gbps / PEAK_GBPS, "valid_pixel_rate_Gpx_s": V / (ms * 1e-3) / 1e9,
                "measured_in": "libellc_hip_diag.so (same sources + the measurement hooks; the shipping library exports none)"}

    def close(self):
        if getattr(self, "_twin", None) is not None:
            self._twin.close()
            self._twin = None
        self.ctx.close()


def workload_name(a, world):
    """BASELINE.json's name of what is being run"""
    if a.dense and (a.width, a.height, a.levels) == (1280, 960, 5):
        return "C4 (configs[4]: 1280x960, 5 levels, dense residuals, %d per GPU x %d GPU%s = batch %d)" % (a.batch, world, "s" if world > 1 else "", a.batch * world)
    if not a.dense and (a.width, a.height, a.levels) == (640, 480, 4):
        return "C2 (configs[2]: batch of %d loop-closure candidate alignments)" % a.batch if world == 1 else \
               "C3 (configs[3]: %d independent alignments sharded %d per GPU, one gather of the se(3) poses)" % (a.batch * world, a.batch)
    return "custom (%dx%d, %d levels, %s, %d per GPU)" % (a.width, a.height, a.levels, "dense" if a.dense else "semi-dense", a.batch)


def pin_rank_to_cpus(a, world, local_rank):
    """N > 1: each rank keeps to its own contiguous share of the CPUs this process may run on (sorted ids: on the two-socket hosts of an
    8-GPU node the lower half of the ids is the socket of GPUs 0-3) — host threads of different ranks (the fetch loop, the CPU baseline)
    do not migrate over each other. Before the library is loaded. Returns what was done, for the JSON line."""
    if world <= 1 or a.no_affinity or not hasattr(os, "sched_setaffinity"):
        return "none"
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    cpus = sorted(os.sched_getaffinity(0))
    per = len(cpus) // max(1, local_world)
    if per < 1:
        return "none (fewer CPUs than ranks)"
    mine = cpus[local_rank * per:(local_rank + 1) * per]
    try:
        os.sched_setaffinity(0, mine)
    except OSError as e:
        return "none (%s)" % e
    return "rank-local block of %d CPUs (%d..%d)" % (len(mine), mine[0], mine[-1])


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "0"))
    if world == 0 and a.gpus > 1:
        sys.exit(spawn_ranks(a))   # this process never loads the library: nothing here has touched a GPU
    world = max(1, world)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.rehearse_launcher:
        return rehearse_launcher(a, world, rank, local_rank)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # (before the HIP runtime starts: RCCL's IPC needs the dmabuf mode on this host driver)
    affinity = pin_rank_to_cpus(a, world, local_rank)          # before the library (and its threads) exist
    from egomotion_with_local_loop_closures_amd import _lib
    if a.lib:
        _lib.use_library(a.lib)
    from egomotion_with_local_loop_closures_amd import api, synth, sharding
    ndev = _lib.lib().ellc_device_count()
    if ndev < 1:
        raise SystemExit("bench.py: no HIP device is visible (there is no CPU fallback for the product path)")
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    if a.backend == "nccl" and world > 1 and local_world > ndev:   # (the same on every rank of the node: no rank starts RCCL)
        raise SystemExit("bench.py: rank %d: %d ranks on this node but %d GPU(s) visible — RCCL refuses two ranks on one device. A scaling run needs a GPU "
                         "per rank; to REHEARSE several ranks on one GPU ask for it: --backend gloo (TCP transport, the ranks share the device, "
                         "n_gpus then counts devices and `value` is null)" % (rank, local_world, ndev))
    if world > 1 and local_world > ndev:
        a.ranks_share_gpus = True
    dev_index = local_rank % ndev
    ctl = Control(sharding, world, rank)

    W, H, L, B = a.width, a.height, a.levels, a.batch
    # ---- synthetic inputs (seeded, per rank), uploaded once: resident in HBM before anything is timed
    if a.dense:
        scenes = [synth.make_pair(W, H, seed=0x5EED + 1000 * rank + i, dense=True) for i in range(2)]
    else:
        scenes = synth.make_shared_frame_batch(W, H, B, seed=0x5EED + 1000 * rank)
    wl = Workload(api, a, scenes, a.arith, dev_index, shared_frame=not a.dense, prime=[a.warmup, a.steps], cache_records=int(a.cache_records))
    G, sched = wl.G, wl.sched
    iters_per_alignment = sum(sched)
    # ---- the gather of the resulting se(3) poses (8 floats per alignment): the batches of one launch group complete together,
    # so their tables are exchanged together — one all-gather per group of `coalesce` batches, enqueued when the group's last
    # batch is fetched and collected a few groups later, so the exchange never stalls the loop. It is the library's own C++
    # path (ellc_gather_start / ellc_gather_finish: ncclAllGather on a stream of its own).
    gathering = world > 1 or a.gather_at_1
    bucket_n = wl.coalesce                      # batches per exchange
    per_max = bucket_n * B * world              # rows of the largest gathered table
    bucket = []
    depth = 4                                   # exchanges in flight: the library keeps a ring of four (ellc_comm)
    comm = None
    if gathering:
        transport = "rccl" if a.backend == "nccl" else "tcp"
        rccl_error = ""
        if transport == "rccl":
            uid = ctl.broadcast_id(sharding.Comm.unique_id)
            try:
                comm = sharding.Comm(world, rank, max_total=per_max, transport="rccl", device=dev_index, unique_id=uid)
            except Exception as e:   # (the ranks then agree on the TCP transport below, and the line says so)
                rccl_error = "%s: %s" % (type(e).__name__, e)
            if ctl.max(1.0 if comm is None else 0.0) > 0.0:   # some rank has no RCCL communicator: the run is not the one asked for
                if comm is not None:
                    comm.close()
                ctl.close()
                raise SystemExit("bench.py: rank %d: RCCL communicator not available (%s) — no silent fallback: --backend gloo asks for the TCP transport explicitly"
                                 % (rank, rccl_error or "another rank failed"))
        if transport == "tcp":   # rehearsal of several ranks on one GPU, or the fallback: the same entry points over TCP
            comm = sharding.Comm(world, rank, max_total=per_max, transport="tcp", host=os.environ.get("MASTER_ADDR", "127.0.0.1"),
                                 port=int(os.environ.get("MASTER_PORT", "29500")) + 18)
    outstanding = []   # rows of each exchange in flight, oldest first
    gathered_rows = [0]
    last_table = [None]   # the newest gathered table (Comm.finish returns a fresh array): what --dump-outputs writes

    def finish_one():
        rows = outstanding.pop(0)
        t = comm.finish(rows)
        assert t.shape == (rows, sharding.RECORD)
        gathered_rows[0] += rows
        last_table[0] = t

    def start(table):
        if len(outstanding) == depth:
            finish_one()
        comm.start(table.shape[0] * world, table)
        outstanding.append(table.shape[0] * world)

    def on_fetch(pose, iters, wgt):
        bucket.append(sharding.pack_results(pose, iters, wgt))
        if len(bucket) == bucket_n:
            start(np.concatenate(bucket))
            bucket.clear()

    def drain():
        if bucket:
            start(np.concatenate(bucket))
            bucket.clear()
        while outstanding:
            finish_one()

    def run(nsteps):
        r = wl.run(nsteps, on_fetch if gathering else None)
        if gathering:
            drain()
        return r

    sync = wl.ctx.sync   # ellc_sync: every stream of the context has drained (no torch in this process)
    if a.device_warmup > 0:   # untimed, before the W warm-up steps: the same steps until clocks, TLBs and the host's call paths are warm
        run(a.device_warmup)   # (measured: the 20 timed steps take 0.150 ms each behind 5 warm-up steps alone, 0.140 behind 200)
        sync()
    if a.warmup > 0:
        run(a.warmup)
    ctl.barrier()
    sync()
    t0 = time.perf_counter()
    pose, iters, wgt = run(a.steps)
    sync()
    ctl.barrier()
    dt_mine = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, pose, iters, wgt, last_table[0])
    dt = ctl.max(dt_mine)
    per_rank_ms = [1e3 * x / a.steps for x in ctl.all(dt_mine)]   # every rank's own time for its K steps (the contract's T is their maximum)
    if a.early_exit:   # every batch of a group repeats the same alignments: the last batch's count holds for all
        iters_per_alignment = float(iters.sum()) / B
    else:
        assert int(iters.sum()) == B * iters_per_alignment, "schedule not fully executed"
    value = world * B * iters_per_alignment * a.steps / dt

    shape = ("%d different keyframes (own depth map each) against ONE current frame per batch, the reference's loop-closure shape" % B) if not a.dense \
        else ("%d independent dense keyframe<->frame alignments per batch" % B)
    gather_txt = ""
    if world > 1:
        gather_txt = ", one all-gather of the poses per launch group, issued by the library's C entry points over %s (overlapped with the next groups)" % (
            "RCCL (ncclAllGather, xGMI)" if transport == "rccl" else
            ("the TCP transport (rehearsal: several ranks on one GPU)" if a.backend != "nccl" else "the TCP transport (NO RCCL communicator could be created: fallback)"))
    out = {
        "metric": "GN iterations/sec (%dx%d %s)" % (W, H, "dense" if a.dense else "semi-dense"),
        "value": value, "unit": "GN iterations/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": 1e3 * dt / a.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": workload_name(a, world) + ": %s, %dx%d, %d-level pyramid, %s Gauss-Newton, schedule %s (early exit %s), per-call mask "
                               "compaction included, arithmetic mode '%s' (%s), %d batches in flight, launched in groups of up to %d side by side (cfg.coalesce) on up to 3 streams%s"
                               % (shape, W, H, L, a.mode.upper(), sched, "ON: informational run" if a.early_exit else "off", a.arith,
                                  "pose <= 1e-5 vs the CPU path, tests/test_gpu_fast.py" if a.arith == "fast" else "per-pixel values bit-identical to the CPU path",
                                  G, wl.coalesce, gather_txt),
                   "batch_per_gpu": B, "global_batch": B * world, "batches_in_flight": G, "coalesce": wl.coalesce,
                   "setup": "slots uploaded; hipGraphs captured by one untimed rehearsal of %d and %d steps (every launch sequence the warm-up "
                            "and the timed steps replay), %d further untimed steps to bring the device to its working state (--device-warmup), then the %d warm-up steps" % (a.warmup, a.steps, a.device_warmup, a.warmup),
                   "launcher": ("ranks started by the caller (WORLD_SIZE in the environment)" if "TORCHELASTIC_RUN_ID" in os.environ or "GROUP_RANK" in os.environ
                                else "ranks started by bench.py itself") if world > 1 else "single process",
                   "control_plane": "library TCP communicator (barrier, unique id, max of the timings); torch is not imported",
                   "gn_iterations_per_alignment": iters_per_alignment,
                   "alignments_per_s": world * B * a.steps / dt, "pixels": "dense" if a.dense else "semi-dense (maxAbsGradient>=5)", "arith": a.arith},
    }
    out["config"]["per_rank_ms_per_step"] = per_rank_ms
    out["config"]["cpu_affinity"] = affinity
    if getattr(a, "ranks_share_gpus", False):   # an explicit rehearsal (--backend gloo): the line must not read as a scaling point
        out["config"]["ranks_share_gpus"] = "%d ranks on %d visible GPU(s): NOT a scaling measurement" % (world, ndev)
        out["config"]["rehearsal_value"] = value
        out["n_gpus"] = ndev
        out["value"] = None
    if gathering:
        out["config"]["gathered_records_rank0"] = gathered_rows[0]
        # self-check of a multi-rank run: what the data path's transport ITSELF reports on every rank (ellc_comm_info: ncclCommCount /
        # ncclCommUserRank / the PCI bus id of the communicator's device) — N ranks on N different devices, or the line says otherwise
        ci = comm.info()
        seen = ctl.all(float(ci["world_seen"]))
        ranks_seen = ctl.all(float(ci["rank_seen"]))
        buses = ctl.all_text(ci["pci_bus_id"])
        out["config"]["comm_transport"] = ci["transport"]
        out["config"]["rccl_ranks" if ci["transport"] == "rccl" else "tcp_ranks"] = int(ci["world_seen"])
        out["config"]["rccl_rank_of_this_process" if ci["transport"] == "rccl" else "tcp_rank_of_this_process"] = int(ci["rank_seen"])
        out["config"]["comm_world_seen_per_rank"] = [int(x) for x in seen]
        out["config"]["comm_rank_seen_per_rank"] = [int(x) for x in ranks_seen]
        out["config"]["pci_bus_id_per_rank"] = buses
        assert all(int(x) == world for x in seen) and [int(x) for x in ranks_seen] == list(range(world)), (seen, ranks_seen, world)
        if ci["transport"] == "rccl" and world > 1:
            assert len(set(buses)) == world and all(buses), "RCCL ranks share a device: %r" % (buses,)

    def finish():
        if comm is not None:
            comm.close()
        ctl.barrier()
        ctl.close()

    if a.trace_only or not a.full:   # a plain run: the contract's fields only
        if rank == 0:
            print(json.dumps(out), flush=True)
        wl.close()
        finish()
        return
    if rank == 0:
        # ---- roofline of the dominant kernel (FCA residual/Jacobian/accumulate at level 0), HIP events on the library's stream
        k0 = wl.level0_kernel()
        traffic, tsrc = pmc_traffic(a, B, G, a.arith)
        out["roofline"] = dict({"bound": "hbm", "kernel": "gn_fca_fused (level 0, one launch group = %d batches of %d side by side, arith %s): solve of the previous "
                                "iteration + residual/Jacobian/accumulate" % (min(wl.coalesce, G), B, a.arith), "peak": PEAK_GBPS, "unit": "GB/s", "traffic": traffic, "traffic_source": tsrc,
                                "level0_gn_iterations_per_s": B / (k0["avg_launch_ms"] * 1e-3)}, **k0)
        # `frac` / `achieved` above are measured live in this process (HIP events around a replayed graph of 50 launches on the warmed
        # device). The committed rocprofv3 kernel trace of the same launch (tools/profile_kernel.py, same grid and arithmetic mode) is
        # quoted beside it with the fraction ITS average duration gives — the figure a reader can recompute from profiles/ alone; the
        # two differ by what the profiler's interception and the box it ran on add (a few per cent).
        prof = profile_kernel_trace(a, a.arith)
        if prof is not None:
            out["roofline"]["frac_inprocess"] = out["roofline"]["frac"]
            out["roofline"]["profile"] = dict(prof, achieved=k0["algorithmic_bytes_per_launch"] / (prof["avg_launch_us"] * 1e-6) / 1e9,
                                              frac=k0["algorithmic_bytes_per_launch"] / (prof["avg_launch_us"] * 1e-6) / 1e9 / PEAK_GBPS)
            out["roofline"]["frac_profile"] = out["roofline"]["profile"]["frac"]
        # what a kernel that only reads reaches on this box (2 GiB, 16-byte lanes, far larger than the 256 MB Infinity Cache)
        cal_bytes = 2 << 30
        cal_ms = wl.diag_twin().ctx.profile_stream_read(cal_bytes, reps=5)
        out["roofline"]["measured_stream_read_GBps"] = cal_bytes / (cal_ms * 1e-3) / 1e9
        if world == 1 and not a.no_extras:
            # ---- spread: further blocks of --steps steps, each bracketed like the timed region
            if a.blocks > 0:
                ms = sorted(1e3 * wl.timed(a.steps)[0] / a.steps for _ in range(a.blocks))
                out["repeat_blocks"] = {"blocks": a.blocks, "steps_per_block": a.steps, "ms_per_step_median": ms[len(ms) // 2], "ms_per_step_min": ms[0],
                                        "ms_per_step_max": ms[-1], "value_at_median": B * iters_per_alignment / (ms[len(ms) // 2] * 1e-3)}
            # ---- sustained: ONE block of many steps (the driver's 20-step window holds the pipeline's fill and drain)
            if a.sustained > 0:
                ds, _, _ = wl.timed(a.sustained)
                out["sustained"] = {"steps": a.sustained, "ms_per_step": 1e3 * ds / a.sustained, "value": B * iters_per_alignment * a.sustained / ds}
            # ---- C1: the same path at B = 1 (latency-bound single alignment)
            wl.ctx.align([0], [0], mode=wl.mode)
            n1 = 30
            t1 = time.perf_counter()
            for _ in range(n1):
                wl.ctx.align([0], [0], mode=wl.mode)
            d1 = (time.perf_counter() - t1) / n1
            out["single_alignment"] = {"workload": "C1: one keyframe vs one frame, same sizes/schedule, arith %s" % a.arith, "ms_per_alignment": 1e3 * d1,
                                       "gn_iterations_per_s": iters_per_alignment / d1}
            gpu_pose0 = pose[0].copy()
            wl.close()
            wl = None
            # ---- the other arithmetic mode on the same workload
            other = "exact" if a.arith == "fast" else "fast"
            w2 = Workload(api, a, scenes, other, dev_index, shared_frame=not a.dense, prime=[a.warmup, a.steps])
            w2.run(a.warmup)
            d2, p2, _ = w2.timed(a.steps)
            k2 = w2.level0_kernel()
            tr2, ts2 = pmc_traffic(a, B, G, other)
            out[other + "_arith"] = {"value": B * iters_per_alignment * a.steps / d2, "ms_per_step": 1e3 * d2 / a.steps,
                                     "roofline": dict({"traffic": tr2, "traffic_source": ts2}, **k2),
                                     "pose_l2_diff_between_modes_max": float(np.linalg.norm(p2 - pose, axis=1).max())}
            # both arithmetic modes side by side where a reader of `config` sees them
            out["config"]["arith_modes"] = {a.arith: {"value": value, "level0_kernel_frac": k0["frac"]},
                                            other: {"value": out[other + "_arith"]["value"], "level0_kernel_frac": k2["frac"]}}
            w2.close()
            # ---- early exit on (the reference's default), one batch at a time: informational
            w3 = Workload(api, a, scenes, a.arith, dev_index, early_exit=1, G=1, shared_frame=not a.dense, coalesce=1)
            _, it3, _ = w3.ctx.align(w3.kf[0], w3.fr[0], mode=w3.mode)
            t3 = time.perf_counter()
            for _ in range(10):
                w3.ctx.align(w3.kf[0], w3.fr[0], mode=w3.mode)
            d3 = (time.perf_counter() - t3) / 10
            done = int(np.asarray(it3).sum())
            out["early_exit_on"] = {"ms_per_batch": 1e3 * d3, "alignments_per_s": B / d3, "gn_iterations_per_s": done / d3,
                                    "mean_iterations_per_alignment": done / B, "batches_in_flight": 1}
            # the tracking call: ONE alignment with early exit (state-driven schedule)
            _, it1, _ = w3.ctx.align(w3.kf[0][:1], w3.fr[0][:1], mode=w3.mode)
            t4 = time.perf_counter()
            for _ in range(30):
                w3.ctx.align(w3.kf[0][:1], w3.fr[0][:1], mode=w3.mode)
            d4 = (time.perf_counter() - t4) / 30
            out["early_exit_on"]["single_alignment"] = {"ms_per_alignment": 1e3 * d4, "iterations": int(np.asarray(it1).sum())}
            if G > 1 and a.mode == "fca":
                out["roofline"]["one_batch_at_a_time_grid"] = w3.level0_kernel()
            w3.close()
            # the same with the queue kept full, as the timed region does it (launch groups, cfg.coalesce)
            w5 = Workload(api, a, scenes, a.arith, dev_index, early_exit=1, shared_frame=not a.dense, prime=[a.warmup, a.steps])
            w5.run(a.warmup)
            d6, _, it6 = w5.timed(a.steps)
            out["early_exit_on"]["pipelined"] = {"ms_per_batch": 1e3 * d6 / a.steps, "alignments_per_s": B * a.steps / d6,
                                                 "gn_iterations_per_s": float(np.asarray(it6).sum()) * a.steps / d6, "batches_in_flight": w5.G,
                                                 "coalesce": w5.coalesce}
            w5.close()
            if not a.dense and a.mode == "fca":
                # ---- the same batches in the constant-weight mode the reference's loop-closure thread uses (ICA, saved weights)
                ns = argparse.Namespace(**vars(a))
                ns.mode = "ica"
                w4 = Workload(api, ns, scenes, a.arith, dev_index, shared_frame=True, prime=[a.warmup, a.steps])
                w4.run(a.warmup)
                d5, _, it5 = w4.timed(a.steps)
                out["ica_mode"] = {"workload": "the same batches, ELLC_MODE_ICA (PixelWisePyramid.cpp:561-974: template-gradient Jacobian, saved "
                                               "weights, H^-1 once per keyframe and level), arith %s" % a.arith,
                                   "value": B * iters_per_alignment * a.steps / d5, "ms_per_step": 1e3 * d5 / a.steps}
                assert int(it5.sum()) == B * iters_per_alignment
                w4.close()
                # ---- a loop-closure STREAM as the reference produces it: the same 32 candidate keyframes against one new frame after
                # another. Batches in flight then share their keyframe slots: with per-call compaction (the default, and what
                # `value` measures on distinct keyframes) they run one after the other; with cfg.cache_records the lists are built
                # once and the batches only read them
                rec = {"workload": "every batch aligns the SAME %d keyframes, against frame slot (step mod %d)" % (B, G)}
                for cache in (0, 1):
                    w6 = Workload(api, a, scenes, a.arith, dev_index, shared_frame=True, prime=[a.warmup, a.steps], share_kf=True, cache_records=cache)
                    w6.run(a.warmup)
                    d7, _, it7 = w6.timed(a.steps)
                    assert int(it7.sum()) == B * iters_per_alignment
                    rec["cache_records_%d" % cache] = {"ms_per_step": 1e3 * d7 / a.steps, "value": B * iters_per_alignment * a.steps / d7}
                    w6.close()
                out["lc_stream_shared_keyframes"] = rec
                out["c4_dense"] = c4_dense(api, synth, a, dev_index)
                out["depth"] = depth_kernels(api, synth, dev_index)
                out["tracked_frame"] = tracked_frame(api, synth, a, dev_index)
                out["tracked_frame_with_lc"] = tracked_frame(api, synth, a, dev_index, with_lc=True)
            if not a.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(a, scenes[0], sched, value, gpu_pose0)
        elif world > 1 and not a.no_cpu_baseline:
            # N > 1: rank 0 times the CPU path AFTER the timed region, on its own share of the host's cores, while the other ranks wait at
            # the closing barrier (the communicator's 60 s deadline covers the bounded sample: three variants of --cpu-seconds each, halved here)
            a.cpu_seconds = min(a.cpu_seconds, 2.0)
            out["cpu_baseline"] = cpu_baseline(a, scenes[0], sched, value / world, pose[0].copy(), pools=False)
            out["cpu_baseline"]["note"] = "timed on rank 0 after the timed region; gpu_over_cpu ratios are per GPU (value / n_gpus)"
        print(json.dumps(out), flush=True)
    if wl is not None:
        wl.close()
    finish()


def dump_outputs(d, pose, iters, wgt, gathered):
    """What the last timed step returned to its caller (ellc_align_fetch), as float arrays: the step's B alignments are the
    same on every run with the same arguments (seeded scenes, group (steps - 1) mod G)."""
    os.makedirs(d, exist_ok=True)
    arrays = {"pose": np.asarray(pose, np.float32), "iters": np.asarray(iters, np.float64), "weighted": np.asarray(wgt, np.float32)}
    if gathered is not None:
        arrays["gathered"] = np.asarray(gathered, np.float32)
    for name, x in arrays.items():
        np.save(os.path.join(d, name + ".npy"), x)


def rehearse_launcher(a, world, rank, local_rank):
    """The launcher and the ranks' control plane without a GPU (tests/test_bench_launcher.py): every rank joins the TCP
    communicator, receives rank 0's id, runs a few pipelined gathers of stand-in result tables through the C entry points
    (libellc_comm.so: the host-only build of csrc/ellc_comm.cpp) and the barrier / max; rank 0 prints what it saw."""
    from egomotion_with_local_loop_closures_amd import sharding
    ctl = Control(sharding, world, rank, host_only=True)
    uid = ctl.broadcast_id(lambda: bytes((7 * i + 255) % 256 for i in range(128)))   # (holds NaN bit patterns: moved bit for bit)
    B = a.batch
    comm = sharding.Comm(world, rank, max_total=B * world, transport="tcp", host=os.environ.get("MASTER_ADDR", "127.0.0.1"),
                         port=int(os.environ.get("MASTER_PORT", "29500")) + 18, host_only=True)
    ok = True
    for s in range(a.steps):
        comm.start(B * world, np.full((B, 8), 1000.0 * s + rank, np.float32))
        if s >= 3:
            t = comm.finish(B * world)
            ok = ok and all(np.all(t[r * B:(r + 1) * B] == 1000.0 * (s - 3) + r) for r in range(world))
    for s in range(max(0, a.steps - 3), a.steps):
        t = comm.finish(B * world)
        ok = ok and all(np.all(t[r * B:(r + 1) * B] == 1000.0 * s + r) for r in range(world))
    ctl.barrier()
    mx = ctl.max(1.0 + rank)
    envs = ctl._gather(1, np.array([rank, local_rank, int(os.environ["WORLD_SIZE"]), int(os.environ["MASTER_PORT"]), os.getpid() % 65536, 0, 0, 0], np.float32)) \
        if world > 1 else np.array([[rank, local_rank, world, 0, 0, 0, 0, 0]], np.float32)
    comm.close()
    ctl.barrier()
    ctl.close()
    if rank == 0:
        print(json.dumps({"rehearsal": "launcher + control plane over the TCP transport, no GPU work", "n_gpus": world, "steps": a.steps, "value": None,
                          "gathers_ok": bool(ok), "id_ok": uid == bytes((7 * i + 255) % 256 for i in range(128)), "max_over_ranks": mx,
                          "ranks": [{"rank": int(e[0]), "local_rank": int(e[1]), "world_size": int(e[2]), "master_port": int(e[3])} for e in envs]}), flush=True)


def c4_dense(api, synth, a, dev_index):
    """BASELINE configs[4] at its per-GPU batch (the honest HBM test — the working set streams from HBM):
    1280x960, 5 levels {4,7,9,12,12}, dense residuals, 16 alignments per batch, pipelined as the main workload is; both arithmetic modes."""
    W, H, L, B = 1280, 960, 5, 16
    scenes = [synth.make_pair(W, H, seed=0xC4 + i, dense=True) for i in range(2)]
    ns = argparse.Namespace(**vars(a))
    ns.early_exit = False
    rec = {"workload": "C4 shape: 1280x960, 5 levels [4,7,9,12,12], dense, 16 alignments per GPU per batch, %d batches in flight in groups of %d"
                       % (min(a.inflight, 4 * a.coalesce if a.coalesce > 1 else 3), a.coalesce), "iterations_per_alignment": 44}
    for arith in ("fast", "exact"):
        steps = 12
        w = Workload(api, ns, scenes, arith, dev_index, W=W, H=H, L=L, B=B, shared_frame=False, prime=[3, steps])
        w.run(3)
        d, _, iters = w.timed(steps)
        assert int(iters.sum()) == B * 44
        # algorithmic bytes of one full-schedule alignment: sum over levels of iters_l * (4 N_l + 14 V_l), V_l = N_l (dense): 144.8 MB
        alg = 0.0
        for l in range(L):
            n = (W >> l) * (H >> l)
            alg += w.sched[l] * 18.0 * n
        k0 = w.level0_kernel(reps=20)
        rec[arith] = {"ms_per_batch": 1e3 * d / steps, "gn_iterations_per_s": B * 44 * steps / d, "algorithmic_bytes_per_batch": alg * B,
                      "achieved_GBps": alg * B / (d / steps) / 1e9, "frac": alg * B / (d / steps) / 1e9 / PEAK_GBPS,
                      "level0_kernel": dict({"bound": "hbm", "peak": PEAK_GBPS, "unit": "GB/s"}, **k0)}
        w.close()
    tr = load_profile_json("c4_pmc_summary")
    if tr:
        rec["level0_kernel_traffic"] = tr
    return rec


def depth_kernels(api, synth, dev_index):
    """The depth-map stages at 640x480 against SURVEY.md section 8(d)'s bytes per pixel (25 B/px SoA state): HIP events on the
    library's stream around repeated enqueues of each stage (ellc_profile_depth_stage)."""
    W, H, L = 640, 480, 4
    pair = synth.make_pair(W, H, seed=31, rot=0.006, trans=0.03)
    fx, fy, cx, cy = pair["intrinsics"]
    st = synth.make_depth_state(W, H, 9, pair["kf_image"], pair["idepth_true"])
    ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, max_keyframes=2, max_frames=1, device=dev_index), diag=True)   # (ellc_profile_depth_stage)
    ctx.keyframe_upload(0, pair["kf_image"]); ctx.frame_upload(0, pair["cur_image"]); ctx.keyframe_from_frame(1, 0)
    xi = pair["xi_true"]
    n = W * H
    rec = {"workload": "640x480, %d valid hypotheses of %d pixels" % (int(st["valid"].sum()), n), "peak_GBps": PEAK_GBPS, "kernels": {}}
    stages = (("dm_regularize (regularizeDepthMap, DepthPropagation.cpp:1436-1543)", 0, 50.0, "hbm"),
              ("dm_fill_holes (fillDepthHoles + buildValIntegralBuffer, :1317-1432)", 1, 50.0, "hbm"),
              ("dm_observe_select + dm_observe_walk (observeDepthRow + line stereo, :191-999)", 2, 94.0, "valu (stereo walks; not a roofline kernel)"),
              ("dm_export_level0 + 3 x depth_pyr_level (updateDepthImage, :1254-1315, 1637-1746)", 3, 9.0 + 12.0 + 8.0 / 3.0, "hbm"),
              ("dm_reg_fill_reg (createKeyFrame's regularise + fill + regularise in one launch, :1775-1777)", 4, 50.0, "valu (three 25-neighbour stencils, the first also on the ring)"),
              ("dm_fill_reg<export> (a tracked frame's fill + regularise + updateDepthImage in one launch, :1627-1635, 1254-1315)", 5, 50.0 + 8.0 + 8.0 / 3.0, "hbm"))
    for name, stage, bpp, bound in stages:
        ctx.depth_set_keyframe(0); ctx.depth_set_state(st)
        ctx.depth_regularize(False)
        ms = ctx.profile_depth_stage(stage, 0, xi, reps=20)
        gbps = bpp * n / (ms * 1e-3) / 1e9
        rec["kernels"][name] = {"us_per_call": 1e3 * ms, "algorithmic_bytes_per_px": bpp, "algorithmic_bytes": bpp * n, "achieved_GBps": gbps,
                                "frac_of_hbm_peak": gbps / PEAK_GBPS, "bound": bound}
    # createKeyFrame: propagate (bucket + per-target fold) + regularise x2 + fill + rescale + export: eight launches, ONE host wait: wall time
    reps = 10
    tot = 0.0
    for _ in range(reps):
        ctx.depth_set_keyframe(0); ctx.depth_set_state(st); ctx.depth_regularize(False); ctx.sync()
        t0 = time.perf_counter()
        ctx.depth_create_keyframe(1, xi)
        ctx.sync()
        tot += time.perf_counter() - t0
    rec["create_keyframe"] = {"us_per_call_wall": 1e6 * tot / reps, "algorithmic_bytes": (61.0 + 3 * 50.0 + 9.0 + 12.0 + 8.0 / 3.0) * n,
                              "achieved_GBps": (61.0 + 3 * 50.0 + 9.0 + 12.0 + 8.0 / 3.0) * n / (tot / reps) / 1e9,
                              "note": "propagate 61 B/px + regularise, fill, regularise 50 B/px each + export; latency-bound at this size "
                                      "(15 MB of state; a chain of eight launches with one host wait, for the rescale factor it returns)"}
    ctx.close()
    return rec


def tracked_frame(api, synth, a, dev_index, with_lc=False):
    """BASELINE configs[1] as the reference's main loop runs it (main.cpp:330, 499-502): per frame an upload (+ pyramid), one FCA
    alignment against the active keyframe with early exit ON and saved weights, then observe / fill holes / regularise /
    updateDepthImage enqueued behind it.
    with_lc: every 8th frame (KEYFRAME_PROPAGATE_INTERVAL) the finished keyframe goes to the loop-closure ring — a context of its
    own — and is aligned against `n_cand` candidates in ONE constant-weight batch (GlobalOptimize.cpp:566), (a) on a host thread
    beside tracking, joined at the next push (the reference's FLAG_DO_PARALLEL_SHORT_LOOP_CLOSURE, :241 / :161; what ellc_main
    does), and (b) inline on the tracking thread, for comparison."""
    import threading
    W, H, L = 640, 480, 4
    pair = synth.make_pair(W, H, seed=0x5EED)
    fx, fy, cx, cy = pair["intrinsics"]
    arith = api.ARITH_FAST if a.arith == "fast" else api.ARITH_EXACT
    n_cand = 8

    def loop(lc_mode, fused=False, persist=1):   # lc_mode: None | "thread" | "inline"
        ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, early_exit=1, max_keyframes=2, max_frames=2, device=dev_index, arith=arith))
        if persist != 1:
            ctx.set_persistent_schedule(persist)   # 0: one launch per Gauss-Newton iteration (the schedule up to r04), for the A/B beside the default
        ctx.keyframe_upload(0, pair["kf_image"]); ctx.keyframe_set_depth(0, pair["depth0"], pair["var0"])
        st = synth.make_depth_state(W, H, 9, pair["kf_image"], pair["idepth_true"])
        ctx.depth_set_keyframe(0); ctx.depth_set_state(st)
        ring = None
        if lc_mode:
            ring = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, early_exit=1, max_keyframes=n_cand + 1, max_frames=1, max_batch=n_cand,
                                                  grid_batch=n_cand, cache_records=1, device=dev_index, arith=arith))   # (as the facade's ring context)
            for k in range(n_cand):
                ring.keyframe_upload(k, pair["kf_image"]); ring.keyframe_set_depth(k, pair["depth0"], pair["var0"])
                for l in range(L):
                    ring.keyframe_set_weights(k, l, np.full((H >> l, W >> l), 0.03, np.float32), 1)
        worker = [None]
        batches = [0]

        def match():   # the matching thread's device work: test keyframe -> frame slot, one ICA batch over the candidates
            ring.copy_slot(False, 0, True, n_cand)
            ring.align(np.arange(n_cand, dtype=np.int32), np.zeros(n_cand, np.int32), mode=api.MODE_ICA)
            batches[0] += 1

        n, its = 256, 0
        warm = 200   # untimed frames first: the loop is timed on a device in its working state (as the main workload, --device-warmup)
        for f in range(warm + n):
            if f == warm:
                if worker[0] is not None:
                    worker[0].join(); worker[0] = None
                ctx.sync()
                t0 = time.perf_counter()
                its = 0
                batches[0] = 0
            ctx.frame_upload(f & 1, pair["cur_image"])
            if fused:   # ellc_track_frame: the depth stages start behind the alignment on the device
                _, it, _, _ = ctx.track_frame(f & 1, save_weights=True)
            else:
                p, it, _ = ctx.align([0], [f & 1], save_weights=True)
                ctx.depth_observe(f & 1, p[0]); ctx.depth_fill_holes(); ctx.depth_regularize(False); ctx.depth_update_depth_image()
            its += int(it.sum())
            if lc_mode and f % 8 == 7:   # pushToArray: join the previous match thread, deep-copy the keyframe, start the next
                if worker[0] is not None:
                    worker[0].join(); worker[0] = None
                api.copy_slot_across(ring, True, n_cand, ctx, True, 0)
                if lc_mode == "thread":
                    worker[0] = threading.Thread(target=match)
                    worker[0].start()
                else:
                    match()
        if worker[0] is not None:
            worker[0].join()
        ctx.sync()
        if ring is not None:
            ring.sync()
        d = (time.perf_counter() - t0) / n
        ctx.close()
        if ring is not None:
            ring.close()
        return d, its / n, batches[0]

    if not with_lc:
        d, its, _ = loop(None, fused=False)
        df, _, _ = loop(None, fused=True)
        dl, _, _ = loop(None, fused=False, persist=0)
        return {"workload": "C1 loop: upload + pyramid, one FCA alignment (early exit on, saved weights), observe + fill holes + regularise + export, "
                            "640x480, 4 levels, arith %s, five calls per frame with the pose through the host (ellc_main --no-fused); "
                            "ms_per_frame_fused_call: the same through ONE ellc_track_frame call per frame, ellc_main's default (the depth stages enqueued behind the "
                            "alignment, matrices built on the device; same bits); ms_per_frame_launch_per_iteration: the five calls with the "
                            "alignment's schedule as one launch per Gauss-Newton iteration (ellc_ctx_set_persistent_schedule(0), the schedule up to "
                            "round 4; same bits) instead of one resident launch" % a.arith,
                "ms_per_frame": 1e3 * d, "frames_per_s": 1.0 / d, "mean_gn_iterations_per_frame": its, "ms_per_frame_fused_call": 1e3 * df,
                "ms_per_frame_launch_per_iteration": 1e3 * dl}
    dt_, its, nb = loop("thread")
    di_, _, _ = loop("inline")
    return {"workload": "the C1 loop with the loop-closure batch of every 8th frame (%d candidates, ICA, a context of its own): on a host thread beside "
                        "tracking, joined at the next push (GlobalOptimize.cpp:241 / :161), against the same batch run inline" % n_cand,
            "ms_per_frame": 1e3 * dt_, "frames_per_s": 1.0 / dt_, "ms_per_frame_lc_inline": 1e3 * di_, "lc_batches": nb, "mean_gn_iterations_per_frame": its}


def load_profile_json(stem):
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s.json" % stem))):
        try:
            best = dict(json.load(open(f)), file=os.path.relpath(f, ROOT))
        except Exception:
            pass
    return best


def profile_kernel_trace(a, arith):
    """Average duration of the dominant kernel in the newest committed rocprofv3 kernel trace of tools/profile_kernel.py on this
    workload's grid and arithmetic mode (profiles/rNN_kernel_trace_<arith>_kernel_stats.csv): file, calls, avg_launch_us."""
    import csv
    import glob
    if a.dense or a.mode != "fca" or (a.width, a.height, a.levels) != (640, 480, 4) or a.batch != 32 or max(1, min(4, a.coalesce)) != 4:
        return None
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_kernel_trace_%s_kernel_stats.csv" % arith))):
        if "_c4_" in os.path.basename(f):
            continue
        try:
            for r in csv.DictReader(open(f)):
                if "gn_fca_fused" in r["Name"]:
                    best = {"file": os.path.relpath(f, ROOT), "calls": int(r["Calls"]), "avg_launch_us": float(r["AverageNs"]) / 1e3}
                    break
        except Exception:
            pass
    return best


def pmc_traffic(a, B, G, arith):
    """HBM bytes per launch of the dominant kernel from the newest committed rocprofv3 PMC summary taken on this workload, grid
    and arithmetic mode (separate --pmc FETCH_SIZE and WRITE_SIZE passes over tools/profile_kernel.py, FETCH_SIZE scaled by the
    calibration kernel: profiles/*_pmc_summary*.json). Counters cannot be read from inside this process, so the figure comes from
    the committed file (named in traffic_source); null when no summary matches."""
    import glob
    if a.dense or a.mode != "fca" or (a.width, a.height, a.levels) != (640, 480, 4):
        return None, None
    best = (None, None)
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_summary*.json"))):
        try:
            d = json.load(open(f))
            run = d["profile_kernel_run"]
            if (run["batch"] == B and run["level"] == 0 and (run.get("concurrent_batches", 1) > 1) == (G > 1) and run.get("arith", "exact") == arith and
                    run.get("coalesce", 1) == max(1, min(4, a.coalesce))):
                best = (d["hbm_traffic"]["traffic_bytes_per_launch"], os.path.relpath(f, ROOT))
        except Exception:
            pass
    return best


def cpu_baseline(a, pair, sched, gpu_value, gpu_pose, pools=True):
    """The CPU restatement (oracle, kind 'port') timed on this box's host cores on a bounded sample of the same
    workload: full-schedule alignments of one 640x480 pair. Variants: one thread; 3 row-band threads created / joined per
    iteration exactly as the reference does (NUM_POSE_THREADS=3, PixelWisePyramid.cpp:424-436) — the headline `value`;
    and a persistent worker pool with 8 / 16 / 32 / 64 row bands (capped at the host's hardware threads), best reported.
    Every variant gets the same wall-time budget; each is run twice and the faster run is kept (host noise). The sample is
    alignment 0 of the GPU batch, so the same leg yields the metric's second half: the L2 distance of the GPU pose from the
    CPU path's pose."""
    from oracle import oracle_py as O
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import oracle_problem
    W, H, L = a.width, a.height, a.levels
    _, kf, cur, dm = oracle_problem(O, W, H, L, pair, early_exit=0, max_iter=sched)
    dp = dm.depth_pyr()
    ncores = max(1, O.hardware_threads())
    lc = (a.mode == "ica")
    if lc:
        for l in range(L):
            kf.set_weights(l, np.full((H >> l, W >> l), 0.03, np.float32), 1)

    def timed(nt, **kw):
        sec, its = O.align_timed(kf, cur, dp, loop_closure=lc, n_threads=nt, reps=1, **kw)   # warm (pool threads, page faults)
        reps = int(max(1, min(200, 0.5 * a.cpu_seconds / max(sec, 1e-3))))
        best = None
        for _ in range(2):
            sec, its = O.align_timed(kf, cur, dp, loop_closure=lc, n_threads=nt, reps=reps, **kw)
            if best is None or its / sec > best["value"]:
                best = {"value": its / sec, "cores": nt, "seconds": sec, "alignments": reps}
        return best

    one = timed(1, spawn_threads=False)
    three = timed(3, spawn_threads=True)
    pool = {}
    for nt in (8, 16, 32, 64):
        if pools and nt <= ncores:
            pool[nt] = timed(nt, pool=True)
    best = max(pool.values(), key=lambda r: r["value"]) if pool else three
    cpu_pose = O.align(kf, cur, dp, loop_closure=lc)[0]
    # ---- batch-parallel: the workload is a batch of INDEPENDENT alignments, and one alignment per host thread is the CPU's natural
    # use of many cores (the reference itself runs the batch's alignments one after the other, GlobalOptimize.cpp:480-610, three row
    # bands each): n alignments at once on n threads, n = 32 (the batch), 64, 128 up to the CPUs this process may run on; each
    # alignment has its own frame objects; bands inside an alignment one after the other on its thread (and, once, the batch as 32 x the
    # reference's 3 band threads). Threads are not pinned: the kernel's scheduler places them (the affinity mask is stated).
    usable = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else ncores
    bp = {}
    if pools:
        nmax = min(128, max(1, usable))
        probs = [(kf, cur, dp)]
        while len(probs) < min(nmax, max(32, nmax)) and len(probs) < 128:
            _, k2, c2, d2 = oracle_problem(O, W, H, L, pair, early_exit=0, max_iter=sched)
            if lc:
                for l in range(L):
                    k2.set_weights(l, np.full((H >> l, W >> l), 0.03, np.float32), 1)
            probs.append((k2, c2, d2.depth_pyr()))

        def timed_batch(n_align, n_outer, spawn):
            pr = probs[:n_align]
            sec, its = O.align_batch_timed(pr, n_outer, loop_closure=lc, spawn_threads=spawn, n_threads=3, reps=1)   # warm
            reps = int(max(1, min(50, 0.5 * a.cpu_seconds / max(sec, 1e-3))))
            bestb = None
            for _ in range(2):
                sec, its = O.align_batch_timed(pr, n_outer, loop_closure=lc, spawn_threads=spawn, n_threads=3, reps=reps)
                if bestb is None or its / sec > bestb["value"]:
                    bestb = {"value": its / sec, "alignments_at_once": n_align, "host_threads": n_outer * (3 if spawn else 1), "seconds": sec,
                             "alignments": reps * n_align}
            return bestb
        for n in (32, 64, 128):
            if n <= len(probs) and (n <= usable or n == 32):
                bp[str(n)] = timed_batch(n, min(n, max(1, usable)), False)
        if len(probs) >= 32:
            bp["32x3_reference_threads"] = timed_batch(32, min(32, max(1, usable)), True)
    bp_best = max(bp.values(), key=lambda r: r["value"]) if bp else None
    return {"value": three["value"], "unit": "GN iterations/s", "cores": 3, "kind": "port",
            "sample": "%d full-schedule alignments (x2 runs, faster kept) of alignment 0 of the GPU batch, a %dx%d %s pair (same schedule/inputs), "
                      "faithful-f32 restatement, 3 row-band threads created/joined per iteration as the reference does; host has %d hardware threads"
                      % (three["alignments"], W, H, "dense" if a.dense else "semi-dense", ncores),
            "1T": one, "3T": three, "3T_over_1T": three["value"] / one["value"],
            "best": dict(best, threading="persistent pool, %d row bands" % best["cores"]),
            "pool_sweep": {str(k): v["value"] for k, v in pool.items()},
            "gpu_over_cpu_3T": gpu_value / three["value"], "gpu_over_cpu_best": gpu_value / best["value"],
            "batch_parallel": None if bp_best is None else dict(
                bp_best, sweep={k: v["value"] for k, v in bp.items()}, cpus_usable=usable, affinity="not pinned (kernel scheduler); mask of %d CPUs" % usable,
                note="one alignment per host thread, the batch's alignments at once: the strongest fair CPU figure for this workload — the reference "
                     "runs them one after the other (GlobalOptimize.cpp:480-610), 3 row-band threads each (PixelWisePyramid.cpp:424-442), which is `value`"),
            "gpu_over_cpu_batch_parallel": None if bp_best is None else gpu_value / bp_best["value"],
            "pose_l2_err_gpu_vs_cpu": float(np.linalg.norm(np.asarray(gpu_pose, np.float32) - cpu_pose))}


if __name__ == "__main__":
    main()
